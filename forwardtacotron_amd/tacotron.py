"""MI355X-native Tacotron teacher: drop-in for models/tacotron.py (the model that produces the attentions durations
are extracted from).  Same constructor, module tree, state_dict (254 entries for the singlespeaker config), buffers and
seed-identical initialisation; the teacher-forced forward() and align() run on the package's HIP kernels.

    reference (models/tacotron.py)                 here
    Tacotron.forward(batch), teacher forcing        Tacotron.forward(batch): inference only (no grad, no training mode)
    -- (the same forward in train(), taco_trainer)  Tacotron.forward_train(batch): the training forward, with autograd
    -- (train_tacotron.py:117-136 runs forward)     Tacotron.align(batch): encoder + attention recurrence only
    Tacotron.generate(x, speaker_emb, steps)        Tacotron.generate: B = 1, eval mode, numpy outputs as the reference
    -- (generate takes one sentence)                Tacotron.generate_batch(x, x_len, speaker_emb, steps): a ragged batch,
                                                    every item what generate gives the sentence alone; device tensors

Under teacher forcing the attention recurrence (attn_rnn GRUCell + LSA + context) is closed over
{h_attn, context, cumulative, attention}; nothing from the decoder LSTMs feeds back into it.  So:
  1. encoder (Embedding -> PreNet -> CBHG, model.CBHG's eval path) and the two token projections, one GEMM each;
  2. the decoder PreNet over all S = ceil(steps / r) teacher-forced frames (mel[:, :, i*r - 1], a zero frame at i = 0)
     and the prenet half of the GRU input projection, as batched GEMMs;
  3. ft_taco_attend: all S steps of the recurrence, three launches per step -> attn [B,S,Tx] and, for forward(), the
     history [S,B,512] of [context | h_attn];
  4. forward() only: rnn_input on the history, then each residual LSTMCell as one-direction LSTM recurrence
     (ft_lstm_fwd_uni) behind one input-projection GEMM, the residual adds, mel_proj restricted to the 80 * r rows
     the [:, :, :r] slice keeps, the postnet CBHG and post_proj.

generate() feeds each step's last frame back into the next step's prenet, so the prenet, rnn_input, both LSTMCells and
mel_proj run inside the recurrence: ft_taco_gen_steps enqueues eight launches per decoder step (the prenet and its GRU
input projection, ft_taco_attend's three kernels, rnn_input, res_rnn1, res_rnn2, mel_proj with the stop test) for
GEN_CHUNK steps per call; the host reads the stop step S_out back once per chunk, then runs the postnet on the
S_out * r frames.

generate_batch() runs the same loop for B sentences of x_len[b] tokens (ft_taco_gen_batch_steps, eight launches per
step): the attention kernels mask at t >= x_len[b] (energies, softmax, LSA state and context stop there, attn is exactly
0 past it), the prenet, rnn_input, both LSTMCells and mel_proj run as 16-item products on the f32 MFMA so that a tile of
16 items reads each weight once per step, and the stop rule is applied per item (s_out [B]); stopped items are stepped
on until the slowest stops and masked afterwards.  The encoder (Encoder.forward_lens) and the postnet (_post with
mel_len) run with lengths.  DESIGN.md section 7 has the masking rule and the tile design.

Dropout: the encoder PreNet and the decoder PreNet apply dropout 0.5 when their own `training` flag is set (extraction
mode, train_tacotron.py:118-119, is `model.eval(); model.decoder.prenet.train()`); every other module must be in eval
mode.  Each dropout site draws its seed from torch's default host generator, `torch.randint(0, 2**62, (1,))`, in this
order: encoder.pre_net fc1, encoder.pre_net fc2 (only when encoder.pre_net is training), decoder.prenet fc1,
decoder.prenet fc2 -- so torch.manual_seed(k) reproduces the masks, as it does for the reference's F.dropout.  A site's mask
is ft_dropout's counter-based mask over the site's tensor in its storage order: [B,Tx,256] and [B,Tx,128] for the
encoder, TIME-major [S,B,256] and [S,B,128] for the decoder (the mask of an element is hip.dropout(ones, 0.5, seed)
at the same position).  One mask per site covers all S steps; the reference draws a fresh one per step from torch's
RNG, which cannot be matched bit for bit either way.

Training: forward_train(batch) is forward() with the whole module tree in train(): batch-statistics BatchNorm (running
statistics and num_batches_tracked updated), `step += 1`, and ten random sites.  It returns (mel_outputs, linear,
attn_scores); the first two carry an autograd graph whose nodes are HIP kernel sequences (ops.py for the CBHGs, Linears,
embedding and layouts; taco_ops.py for the PreNet layers, the attention recurrence with its BPTT ft_taco_attend_bwd, the
zoneout LSTMCells ft_taco_lstm_zone_fwd / _bwd and mel_proj), attn_scores is NOT differentiable (the reference's trainer
only scores it, taco_trainer.py:100).  The reference's loop -- optimizer.zero_grad(); loss.backward(); clip_grad_norm_;
optimizer.step() with torch.optim.Adam -- works on the device tensors as it stands, with l1_loss() below for its two
F.l1_loss terms.  Seed order of forward_train, one dropout_seed() per site with p > 0 (a site with p = 0 draws nothing
and is recorded as None): encoder.pre_net.fc1, encoder.pre_net.fc2, encoder.cbhg.bank (behind the pooled bank, the
[B,Tx,K*128] buffer), encoder.cbhg.conv_project1 ([B,Tx,128]), decoder.prenet.fc1, decoder.prenet.fc2 (time-major, as
above), decoder.res_rnn1, decoder.res_rnn2 (zoneout, [S,B,lstm_dims] time-major), postnet.bank ([B,T,K*postnet_dims]),
postnet.conv_project1 ([B,T,256]).  model.last_seeds maps these names to the seeds of the last call, so every mask can
be rebuilt on the host (tests/dropout_cpu.site_mask).  Zoneout (models/tacotron.py:119-122): h_s = m_s h_{s-1} +
(1 - m_s) LSTMCell(x_s, (h_{s-1}, c_{s-1})).h with m = 1 exactly where the site's ft_dropout mask of probability
model.zoneout (a plain attribute, 0.1, not in the state_dict) is 0 -- P(m = 1) = p, no rescaling; the cell state is not
zoned, the zoned h is the residual output and the next step's recurrent input.  mel_proj runs on the 80 * r rows the
[:, :, :r] slice keeps and its gradient has exact zeros in the other rows; attn_rnn.weight_ih gets one [768,384] gradient,
columns :256 from the recurrence and 256: from the batched prenet projection.
"""
import math
from pathlib import Path
from typing import Any, Dict, Tuple, Union

import torch
import torch.nn as nn

from . import _lib
from . import hip as H
from . import ops
from . import taco_ops as TO
from .hip import _p, _stream
from .base import PAD_VALUE
from .model import CBHG

NUM_CHARS_DEFAULT = 135      # len(utils.text.symbols.phonemes)
MAX_TX = 1024                # ft_taco_attend's token bound (the duration kernel's)
GEN_CHUNK = 32               # decoder steps per ft_taco_gen_steps / ft_taco_gen_batch_steps call (outputs do not depend on it)

FtError = _lib.FtError


def dropout_seed() -> int:
    """seed of one dropout site: one draw from torch's default host generator (see the module docstring)"""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class Encoder(nn.Module):
    """models/tacotron.py:11-26"""

    def __init__(self, embed_dims, num_chars, cbhg_channels, K, num_highways, dropout):
        super().__init__()
        self.embedding = nn.Embedding(num_chars, embed_dims)
        self.pre_net = PreNet(embed_dims)
        self.cbhg = CBHG(K=K, in_channels=cbhg_channels, channels=cbhg_channels,
                         proj_channels=[cbhg_channels, cbhg_channels], num_highways=num_highways)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B,Tx] int64 -> [B,Tx,2*cbhg_channels]"""
        y = H.embedding_fwd(x.contiguous(), self.embedding.weight)
        y = self.pre_net(y)
        return self.cbhg(y)

    def forward_lens(self, x: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """eval forward of a ragged batch: x [B,Tx] int64 (ids at t >= lens[b] are not read), lens int64 [B] on the
        device -> [B,Tx,2*cbhg_channels], every valid row what the item gets alone, zero at t >= lens[b]"""
        if self.training:
            raise FtError('Encoder.forward_lens is the eval-mode (inference) path')
        y = H.embedding_fwd_lens(x.contiguous(), lens, self.embedding.weight)
        y = H.mask_rows(self.pre_net(y), lens)              # the biases make the padded rows non-zero: mask for the CBHG
        return self.cbhg.forward_lens(y, lens)


class PreNet(nn.Module):
    """models/tacotron.py:29-45: fc1 -> ReLU -> dropout -> fc2 -> ReLU -> dropout, over the last dim"""

    def __init__(self, in_dims, fc1_dims=256, fc2_dims=128, dropout=0.5):
        super().__init__()
        self.fc1 = nn.Linear(in_dims, fc1_dims)
        self.fc2 = nn.Linear(fc1_dims, fc2_dims)
        self.p = dropout

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = H.linear_fwd(x, self.fc1.weight, self.fc1.bias, relu=True)
        if self.training and self.p > 0:
            y = H.dropout(y, self.p, dropout_seed())
        y = H.linear_fwd(y, self.fc2.weight, self.fc2.bias, relu=True)
        if self.training and self.p > 0:
            y = H.dropout(y, self.p, dropout_seed())
        return y


class LSA(nn.Module):
    """models/tacotron.py:65-99 (parameter container; the recurrence is ft_taco_attend)"""

    def __init__(self, attn_dim, kernel_size=31, filters=32):
        super().__init__()
        self.conv = nn.Conv1d(2, filters, padding=(kernel_size - 1) // 2, kernel_size=kernel_size, bias=False)
        self.L = nn.Linear(filters, attn_dim, bias=True)
        self.W = nn.Linear(attn_dim, attn_dim, bias=True)
        self.v = nn.Linear(attn_dim, 1, bias=False)


class Decoder(nn.Module):
    """models/tacotron.py:102-174 (parameter container)"""
    max_r = 20

    def __init__(self, n_mels, decoder_dims, lstm_dims):
        super().__init__()
        self.register_buffer('r', torch.tensor(1, dtype=torch.int))
        self.n_mels = n_mels
        self.prenet = PreNet(n_mels)
        self.attn_net = LSA(decoder_dims)
        self.attn_rnn = nn.GRUCell(decoder_dims + decoder_dims // 2, decoder_dims)
        self.rnn_input = nn.Linear(2 * decoder_dims, lstm_dims)
        self.res_rnn1 = nn.LSTMCell(lstm_dims, lstm_dims)
        self.res_rnn2 = nn.LSTMCell(lstm_dims, lstm_dims)
        self.mel_proj = nn.Linear(lstm_dims, n_mels * self.max_r, bias=False)


class Tacotron(nn.Module):
    """Drop-in for models/tacotron.py:177-373 (teacher-forced forward, align, generate and the training forward)."""

    def __init__(self, embed_dims: int, num_chars: int, encoder_dims: int, decoder_dims: int, n_mels: int,
                 postnet_dims: int, encoder_k: int, lstm_dims: int, postnet_k: int, num_highways: int,
                 dropout: float, stop_threshold: float, speaker_emb_dim=256) -> None:
        # the reference only runs with these (PreNet's 128 outputs and the postnet's [256, 80] projection are fixed);
        # the attention kernel is specialised to them
        if encoder_dims != 128 or decoder_dims != 256 or n_mels != 80:
            raise FtError(f'Tacotron: encoder_dims, decoder_dims and n_mels must be 128, 256 and 80, as the reference '
                          f'requires (got {encoder_dims}, {decoder_dims}, {n_mels})')
        super().__init__()
        self.n_mels = n_mels
        self.lstm_dims = lstm_dims
        self.decoder_dims = decoder_dims
        self.encoder = Encoder(embed_dims, num_chars, encoder_dims, encoder_k, num_highways, dropout)
        self.encoder_proj_query = nn.Linear(decoder_dims + speaker_emb_dim, decoder_dims, bias=False)
        self.encoder_proj = nn.Linear(decoder_dims + speaker_emb_dim, decoder_dims, bias=False)
        self.decoder = Decoder(n_mels, decoder_dims, lstm_dims)
        self.postnet = CBHG(postnet_k, n_mels, postnet_dims, [256, 80], num_highways)
        self.post_proj = nn.Linear(postnet_dims * 2, n_mels, bias=False)
        self.speaker_emb_dim = speaker_emb_dim
        self.init_model()
        self.register_buffer('step', torch.zeros(1, dtype=torch.long))
        self.register_buffer('stop_threshold', torch.tensor(stop_threshold, dtype=torch.float32))
        self._packs = {}
        self.zoneout = 0.1           # Decoder.zoneout's p in forward_train (models/tacotron.py:119); not in the state_dict
        self.last_seeds = {}         # site name -> seed of the last forward_train call (None: p = 0, nothing drawn)
        self._forced_seeds = None    # tests: site name -> seed to use instead of a draw

    def __repr__(self):
        return f'Tacotron, num params: {sum(p.numel() for p in self.parameters())}'

    @property
    def r(self) -> int:
        return self.decoder.r.item()

    @r.setter
    def r(self, value: int) -> None:
        self.decoder.r = self.decoder.r.new_tensor(value, requires_grad=False)

    def init_model(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def get_step(self):
        return self.step.data.item()

    def reset_step(self):
        self.step = self.step.data.new_tensor(1)

    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> 'Tacotron':
        model_config = config['tacotron']['model']
        model_config['num_chars'] = config.get('num_chars', NUM_CHARS_DEFAULT)     # reference: len(phonemes)
        model_config['n_mels'] = config['dsp']['num_mels']
        return Tacotron(**model_config)

    @classmethod
    def from_checkpoint(cls, path: Union[Path, str]) -> 'Tacotron':
        checkpoint = torch.load(path, map_location=torch.device('cpu'), weights_only=True)
        model = Tacotron.from_config(checkpoint['config'])
        model.load_state_dict(checkpoint['model'])
        return model

    def generate(self, x: torch.Tensor, speaker_emb: torch.Tensor = None, steps=2000) -> Tuple[Any, Any, Any]:
        """models/tacotron.py:283-349 at B = 1 -> numpy (mel_outputs [80, S_out*r], linear [80, S_out*r],
        attn_scores [S_out, Tx]).  Runs under torch.no_grad(); eval() on entry and train() on return, as the reference.
        The decoder steps run in chunks of GEN_CHUNK (ft_taco_gen_steps), S_out is read back once per chunk."""
        w = self.encoder.embedding.weight
        if not w.is_cuda:
            raise FtError('Tacotron.generate runs on an MI355X (HIP) device only: move the model with .cuda()')
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] != 1:
            raise FtError(f'Tacotron.generate: x must be [1, Tx] (batch size 1, as the reference), got '
                          f'{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
        if not 1 <= x.shape[1] <= MAX_TX:
            raise FtError(f'Tacotron.generate: Tx must be in 1..{MAX_TX} (got {x.shape[1]})')
        steps = int(steps)
        if steps < 1:
            raise FtError(f'Tacotron.generate: steps must be >= 1 (got {steps})')
        if self.speaker_emb_dim > 0 and speaker_emb is not None and tuple(speaker_emb.shape) != (1, self.speaker_emb_dim):
            raise FtError(f'Tacotron.generate: speaker_emb must be [1, {self.speaker_emb_dim}], got '
                          f'{tuple(speaker_emb.shape)}')
        r = self.r
        if not 1 <= r <= Decoder.max_r:
            raise FtError(f'Tacotron.generate: r must be in 1..{Decoder.max_r} (got {r})')
        self.eval()
        try:
            with torch.no_grad():
                if speaker_emb is None and self.speaker_emb_dim > 0:
                    speaker_emb = torch.rand((1, self.speaker_emb_dim))           # the reference's draw
                return self._generate(x.to(w.device, torch.int64).contiguous(), speaker_emb, steps, r)
        finally:
            self.train()

    def _generate(self, x: torch.Tensor, semb, steps: int, r: int):
        dev = x.device
        Tx = x.shape[1]
        S = math.ceil(steps / r)
        D, Ld, n_mels = self.decoder_dims, self.lstm_dims, self.n_mels
        dec = self.decoder
        enc = self.encoder(x)                                                   # [1,Tx,256]
        if self.speaker_emb_dim > 0:
            semb = semb.to(device=dev, dtype=torch.float32).contiguous()
            enc = H.concat_cols(enc, None, semb, 1, Tx)
        ep = H.linear_fwd(enc, self.encoder_proj.weight)
        epq = H.linear_fwd(enc, self.encoder_proj_query.weight)
        f32 = dict(device=dev, dtype=torch.float32)
        P = torch.empty(S, 3 * D, **f32)
        hist = torch.empty(S, 2 * D, **f32)
        attn = torch.empty(1, S, Tx, **f32)
        frames = torch.empty(1, S * r, n_mels, **f32)
        s_out = torch.empty(1, device=dev, dtype=torch.int32)
        nbytes = _lib.query('ft_taco_gen_workspace', Tx, Ld, r)
        if nbytes == 0:
            raise FtError(f'Tacotron.generate: no workspace for Tx = {Tx}, lstm_dims = {Ld}, r = {r}')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        gru, lsa, pn = dec.attn_rnn, dec.attn_net, dec.prenet
        l1, l2 = dec.res_rnn1, dec.res_rnn2
        ops = (_p(ep), _p(epq), _p(pn.fc1.weight), _p(pn.fc1.bias), _p(pn.fc2.weight), _p(pn.fc2.bias),
               _p(gru.weight_ih), gru.weight_ih.shape[1], _p(gru.bias_ih), _p(gru.weight_hh), _p(gru.bias_hh),
               _p(lsa.W.weight), _p(lsa.W.bias), _p(lsa.conv.weight), _p(lsa.L.weight), _p(lsa.L.bias),
               _p(lsa.v.weight), _p(dec.rnn_input.weight), _p(dec.rnn_input.bias),
               _p(l1.weight_ih), _p(l1.weight_hh), _p(l1.bias_ih), _p(l1.bias_hh),
               _p(l2.weight_ih), _p(l2.weight_hh), _p(l2.bias_ih), _p(l2.bias_hh), _p(dec.mel_proj.weight),
               float(self.stop_threshold), _p(P), _p(hist), _p(attn), _p(frames), _p(s_out), Tx, Ld, r, S)
        # chunk c is enqueued before chunk c-1's S_out is waited for: at most one host wait per chunk
        host = torch.empty(2, dtype=torch.int32, pin_memory=True)
        events = [torch.cuda.Event(), torch.cuda.Event()]
        s0, c, n_out = 0, 0, S
        while s0 < S:
            n = min(GEN_CHUNK, S - s0)
            _lib.call('ft_taco_gen_steps', *ops, s0, n, _p(ws), ws.numel(), _stream())
            host[c % 2:c % 2 + 1].copy_(s_out, non_blocking=True)
            events[c % 2].record()
            s0 += n
            if c > 0:
                events[(c - 1) % 2].synchronize()
                n_out = int(host[(c - 1) % 2])
                if n_out < S:
                    break
            c += 1
        else:
            events[(c - 1) % 2].synchronize()
            n_out = int(host[(c - 1) % 2])
        self._gen_steps_run = s0                                                # for tools/bench_taco_generate.py
        T = n_out * r
        mel_cl = frames[:, :T]
        mel_out, lin = self._post(mel_cl)
        return mel_out[0].cpu().numpy(), lin[0].cpu().numpy(), attn[0, :n_out].cpu().numpy()

    # -- generate_batch: the teacher's generate for a ragged batch -----------------------------------------------------
    def generate_batch(self, x: torch.Tensor, x_len: torch.Tensor, speaker_emb: torch.Tensor = None,
                       steps=2000) -> Dict[str, torch.Tensor]:
        """generate() of a RAGGED batch of sentences: for every item b the valid part of the result is what
        generate(x[b:b+1, :x_len[b]], speaker_emb[b:b+1], steps) gives that sentence alone (the
        masking rule), the reference's stop rule applied per item.

        x: int64 [B,Tx]; entries at t >= x_len[b] are ignored, whatever valid symbol ids they hold.  x_len: int64 [B], on
        the host or the device, 1 <= x_len[b] <= Tx <= MAX_TX; a host x_len is range-checked before anything is launched,
        a device x_len out of range raises FtError through a device flag at the end of the call.  speaker_emb: float32
        [B, speaker_emb_dim], one row per item, required when speaker_emb_dim > 0.  steps and self.r hold for the whole
        batch: S = ceil(steps / r) caps every item.

        -> dict of device tensors: mel, linear [B,80,Tm] with Tm = max(mel_len) and base.PAD_VALUE at t >= mel_len[b];
        attn [B,Sm,Tx] with Sm = max(steps_out), exact zeros at t >= x_len[b] and at s >= steps_out[b]; mel_len int64 [B]
        = steps_out * r; steps_out int64 [B].  An item that has stopped is stepped on until the slowest item stops (its
        later slots are masked).  Runs under torch.no_grad(); eval() on entry and train() on return, like generate."""
        w = self.encoder.embedding.weight
        if not w.is_cuda:
            raise FtError('Tacotron.generate_batch runs on an MI355X (HIP) device only: move the model with .cuda()')
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1:
            raise FtError(f'Tacotron.generate_batch: x must be [B, Tx] with B >= 1, got '
                          f'{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
        B, Tx = x.shape
        if not 1 <= Tx <= MAX_TX:
            raise FtError(f'Tacotron.generate_batch: Tx must be in 1..{MAX_TX} (got {Tx})')
        if not torch.is_tensor(x_len) or x_len.dim() != 1 or x_len.numel() != B or x_len.dtype != torch.int64:
            raise FtError(f'Tacotron.generate_batch: x_len must be int64 [B = {B}], got '
                          f'{(tuple(x_len.shape), x_len.dtype) if torch.is_tensor(x_len) else type(x_len).__name__}')
        on_host = not x_len.is_cuda
        if on_host and (int(x_len.min()) < 1 or int(x_len.max()) > Tx):
            raise FtError(f'Tacotron.generate_batch: every x_len must be in [1, Tx = {Tx}] (got {x_len.tolist()})')
        steps = int(steps)
        if steps < 1:
            raise FtError(f'Tacotron.generate_batch: steps must be >= 1 (got {steps})')
        if self.speaker_emb_dim > 0:
            if speaker_emb is None:
                raise FtError(f'Tacotron.generate_batch: speaker_emb_dim = {self.speaker_emb_dim} needs speaker_emb '
                              f'[B, {self.speaker_emb_dim}], one row per item (a random speaker per batch has no meaning)')
            if not torch.is_tensor(speaker_emb) or tuple(speaker_emb.shape) != (B, self.speaker_emb_dim):
                raise FtError(f'Tacotron.generate_batch: speaker_emb must be [{B}, {self.speaker_emb_dim}], got '
                              f'{tuple(speaker_emb.shape) if torch.is_tensor(speaker_emb) else type(speaker_emb).__name__}')
        r = self.r
        if not 1 <= r <= Decoder.max_r:
            raise FtError(f'Tacotron.generate_batch: r must be in 1..{Decoder.max_r} (got {r})')
        self.eval()
        try:
            with torch.no_grad():
                return self._generate_batch(x.to(w.device, torch.int64).contiguous(), x_len, speaker_emb, steps, r)
        finally:
            self.train()

    def _generate_batch(self, x: torch.Tensor, x_len: torch.Tensor, semb, steps: int, r: int):
        dev = x.device
        B, Tx = x.shape
        S = math.ceil(steps / r)
        D, Ld, n_mels = self.decoder_dims, self.lstm_dims, self.n_mels
        dec = self.decoder
        xl = x_len.to(dev).contiguous()
        bad_host = None
        if x_len.is_cuda:
            # the kernels get lengths inside [1, Tx] whatever the tensor holds; the flag is read behind the decoder loop
            bad_host = torch.zeros(1, dtype=torch.bool, pin_memory=True)
            bad_host.copy_(((xl < 1) | (xl > Tx)).any().reshape(1), non_blocking=True)
            xl = xl.clamp(1, Tx)
        enc = self.encoder.forward_lens(x, xl)                                  # [B,Tx,256], zero at t >= x_len[b]
        if self.speaker_emb_dim > 0:
            semb = semb.to(device=dev, dtype=torch.float32).contiguous()
            enc = H.concat_cols(enc, None, semb, B, Tx)                         # one speaker row per item
        ep = H.linear_fwd(enc, self.encoder_proj.weight)
        epq = H.linear_fwd(enc, self.encoder_proj_query.weight)
        f32 = dict(device=dev, dtype=torch.float32)
        P = torch.empty(S, B, 3 * D, **f32)
        hist = torch.empty(S, B, 2 * D, **f32)
        attn = torch.empty(B, S, Tx, **f32)
        frames = torch.empty(B, S * r, n_mels, **f32)
        s_out = torch.empty(B, device=dev, dtype=torch.int32)
        nbytes = _lib.query('ft_taco_gen_batch_workspace', B, Tx, Ld, r)
        if nbytes == 0:
            raise FtError(f'Tacotron.generate_batch: no workspace for B = {B}, Tx = {Tx}, lstm_dims = {Ld}, r = {r}')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        gru, lsa, pn = dec.attn_rnn, dec.attn_net, dec.prenet
        l1, l2 = dec.res_rnn1, dec.res_rnn2
        ops = (_p(ep), _p(epq), _p(pn.fc1.weight), _p(pn.fc1.bias), _p(pn.fc2.weight), _p(pn.fc2.bias),
               _p(gru.weight_ih), gru.weight_ih.shape[1], _p(gru.bias_ih), _p(gru.weight_hh), _p(gru.bias_hh),
               _p(lsa.W.weight), _p(lsa.W.bias), _p(lsa.conv.weight), _p(lsa.L.weight), _p(lsa.L.bias),
               _p(lsa.v.weight), _p(dec.rnn_input.weight), _p(dec.rnn_input.bias),
               _p(l1.weight_ih), _p(l1.weight_hh), _p(l1.bias_ih), _p(l1.bias_hh),
               _p(l2.weight_ih), _p(l2.weight_hh), _p(l2.bias_ih), _p(l2.bias_hh), _p(dec.mel_proj.weight),
               float(self.stop_threshold), _p(P), _p(hist), _p(attn), _p(frames), _p(s_out), _p(xl), B, Tx, Ld, r, S)
        # as _generate: chunk c is enqueued before chunk c-1's s_out [B] is waited for; the loop ends once every item
        # has stopped within the steps already completed
        host = torch.empty(2, B, dtype=torch.int32, pin_memory=True)
        events = [torch.cuda.Event(), torch.cuda.Event()]
        s0, c, last = 0, 0, None
        while s0 < S:
            n = min(GEN_CHUNK, S - s0)
            _lib.call('ft_taco_gen_batch_steps', *ops, s0, n, _p(ws), ws.numel(), _stream())
            host[c % 2].copy_(s_out, non_blocking=True)
            events[c % 2].record()
            s0 += n
            if c > 0:
                events[(c - 1) % 2].synchronize()
                last = host[(c - 1) % 2]
                if int(last.max()) < S:
                    break
            c += 1
        else:
            events[(c - 1) % 2].synchronize()
            last = host[(c - 1) % 2]
        self._gen_batch_steps_run = s0                                          # for tools/bench_taco_generate_batch.py
        if bad_host is not None and bool(bad_host[0]):
            raise FtError(f'Tacotron.generate_batch: every x_len must be in [1, Tx = {Tx}]')
        Sm = int(last.max())
        steps_out = last.clone().to(dev, torch.int64)
        mel_len = steps_out * r
        mel_out, lin = self._post(frames[:, :Sm * r].contiguous(), mel_len)
        return {'mel': mel_out, 'linear': lin, 'attn': H.mask_rows(attn[:, :Sm].contiguous(), steps_out),
                'mel_len': mel_len, 'steps_out': steps_out}

    # ------------------------------------------------------------------------------------------------------------------
    def _check(self, batch) -> Tuple[torch.Tensor, torch.Tensor, Any]:
        dropout_ok = {id(m) for pn in (self.encoder.pre_net, self.decoder.prenet) for m in pn.modules()}
        for name, m in self.named_modules():
            if m.training and id(m) not in dropout_ok:
                raise FtError(f'Tacotron: module {name or "<root>"} is in training mode; forward / align are '
                              'inference paths, training the teacher goes through Tacotron.forward_train (use '
                              'model.eval(), optionally with model.decoder.prenet.train() for the extraction mode of '
                              'train_tacotron.py)')
        w = self.encoder.embedding.weight
        if not w.is_cuda:
            raise FtError('Tacotron runs on an MI355X (HIP) device only: move the model with .cuda()')
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            # as model._eval_needs_no_grad: refuse rather than hand back tensors that silently carry no gradient
            raise FtError('Tacotron.forward / align is an inference path (no autograd graph): call it under '
                          'torch.no_grad(), or with parameters that do not require grad (Tacotron.forward_train is the '
                          'differentiable forward)')
        return self._check_batch(batch)

    def _check_batch(self, batch) -> Tuple[torch.Tensor, torch.Tensor, Any]:
        """the batch conditions of forward / align / forward_train -> (x int64, mel fp32, speaker_emb or None) on the device"""
        w = self.encoder.embedding.weight
        x = batch['x'].to(w.device, non_blocking=True)
        mel = batch['mel'].to(w.device, non_blocking=True)
        if x.dim() != 2 or mel.dim() != 3 or mel.shape[0] != x.shape[0] or mel.shape[1] != self.n_mels:
            raise FtError(f'Tacotron: expected x [B,Tx] and mel [B,{self.n_mels},steps], got {tuple(x.shape)} and '
                          f'{tuple(mel.shape)}')
        if not 1 <= x.shape[1] <= MAX_TX:
            raise FtError(f'Tacotron: Tx must be in 1..{MAX_TX} (got {x.shape[1]})')
        if mel.shape[2] < 1:
            raise FtError('Tacotron: the mel has no frames')
        semb = None
        if self.speaker_emb_dim > 0:
            semb = batch.get('speaker_emb')
            if semb is None:
                raise FtError(f'Tacotron: speaker_emb_dim = {self.speaker_emb_dim} needs batch["speaker_emb"] [B, '
                              f'{self.speaker_emb_dim}]')
            semb = semb.to(device=w.device, dtype=torch.float32, non_blocking=True).contiguous()
            if semb.shape != (x.shape[0], self.speaker_emb_dim):
                raise FtError(f'Tacotron: speaker_emb must be [B, {self.speaker_emb_dim}], got {tuple(semb.shape)}')
        r = self.r
        if not 1 <= r <= Decoder.max_r:
            raise FtError(f'Tacotron: r must be in 1..{Decoder.max_r} (got {r})')
        return x.to(torch.int64).contiguous(), mel.to(torch.float32).contiguous(), semb

    def _pack(self, key, src: torch.Tensor, make):
        """weight-derived operands, rebuilt when the source tensor changes (in-place updates bump _version)"""
        tag = (src.data_ptr(), src._version, src.device)
        hit = self._packs.get(key)
        if hit is None or hit[0] != tag:
            hit = (tag, make())
            self._packs[key] = hit
        return hit[1]

    def _attend_inputs(self, x: torch.Tensor, mel: torch.Tensor, semb):
        """encoder, the two token projections, the decoder prenet over the S teacher-forced frames and the prenet half
        of the GRU input projection -> (enc_proj, enc_pq [B,Tx,256], P [S,B,768])"""
        B, Tx = x.shape
        r = self.r
        steps = mel.shape[2]
        S = math.ceil(steps / r)
        dec = self.decoder
        enc = self.encoder(x)                                                   # [B,Tx,256]
        if semb is not None:
            enc = H.concat_cols(enc, None, semb, B, Tx)                         # [B,Tx,256+S]
        ep = H.linear_fwd(enc, self.encoder_proj.weight)
        epq = H.linear_fwd(enc, self.encoder_proj_query.weight)
        frames = torch.empty(S, B, self.n_mels, device=x.device, dtype=torch.float32)
        _lib.call('ft_taco_frames', _p(mel), B, self.n_mels, steps, r, S, _p(frames), _stream())
        pre = dec.prenet(frames)                                                # [S,B,128]
        gru = dec.attn_rnn
        D = self.decoder_dims
        w_pre = self._pack('w_ih_prenet', gru.weight_ih,
                           lambda: H.slice_cols(gru.weight_ih.detach()[None], D, D // 2)[0])   # W_ih[:, 256:]
        return ep, epq, H.linear_fwd(pre, w_pre, gru.bias_ih)                  # P [S,B,768]

    def _attend(self, ep: torch.Tensor, epq: torch.Tensor, P: torch.Tensor, keep_history: bool):
        """ft_taco_attend -> (attn [B,S,Tx], history [S,B,512] of [context | h_attn], or None)"""
        B, Tx = ep.shape[:2]
        S = P.shape[0]
        gru, lsa = self.decoder.attn_rnn, self.decoder.attn_net
        attn = torch.empty(B, S, Tx, device=ep.device, dtype=torch.float32)
        hist = torch.empty(S, B, 2 * self.decoder_dims, device=ep.device, dtype=torch.float32) if keep_history else None
        _lib.call('ft_taco_attend', _p(ep), _p(epq), _p(P), _p(gru.weight_ih), gru.weight_ih.shape[1],
                  _p(gru.weight_hh), _p(gru.bias_hh), _p(lsa.W.weight), _p(lsa.W.bias), _p(lsa.conv.weight),
                  _p(lsa.L.weight), _p(lsa.L.bias), _p(lsa.v.weight), _p(attn), _p(hist), B, Tx, S,
                  *H.scratch('ft_taco_attend_workspace', B, Tx, device=ep.device), _stream())
        return attn, hist

    def align(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """attn_scores [B, S, Tx] of forward(batch), bit for bit, from the encoder, the decoder prenet and the attention
        recurrence alone (the mel path is not run)."""
        x, mel, semb = self._check(batch)
        attn, _ = self._attend(*self._attend_inputs(x, mel, semb), keep_history=False)
        return attn

    def _lstm(self, cell: nn.LSTMCell, x: torch.Tensor) -> torch.Tensor:
        """nn.LSTMCell over the S steps of x [S,B,L] from zero states -> h [S,B,L]"""
        S, B, Ld = x.shape
        xp = H.linear_fwd(x, cell.weight_ih, cell.bias_ih)                     # [S,B,4L]
        out = torch.empty(S, B, Ld, device=x.device, dtype=torch.float32)
        cst = torch.empty(S, B, Ld, device=x.device, dtype=torch.float32)
        ws, nb = H._rnn_workspace(4, B, Ld, x.device)
        _lib.call('ft_lstm_fwd_uni', _p(xp), _p(cell.weight_hh), _p(cell.bias_hh), _p(out), _p(cst), B, S, Ld, _p(ws),
                  nb, _stream())
        return out

    def _add(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        out = torch.empty_like(x)
        _lib.call('ft_taco_add', _p(x), _p(y), _p(out), x.numel(), _stream())
        return out

    def forward(self, batch: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """models/tacotron.py:219-280 (teacher forcing) -> (mel_outputs [B,80,S*r], linear [B,80,S*r],
        attn_scores [B,S,Tx])"""
        x, mel, semb = self._check(batch)
        attn, hist = self._attend(*self._attend_inputs(x, mel, semb), keep_history=True)
        mel_out, linear = self._mel_path(hist)
        return mel_out, linear, attn

    # -- training ------------------------------------------------------------------------------------------------------
    SITES = ('encoder.pre_net.fc1', 'encoder.pre_net.fc2', 'encoder.cbhg.bank', 'encoder.cbhg.conv_project1',
             'decoder.prenet.fc1', 'decoder.prenet.fc2', 'decoder.res_rnn1', 'decoder.res_rnn2', 'postnet.bank',
             'postnet.conv_project1')

    def _site_p(self) -> Dict[str, float]:
        ep, dp = self.encoder.pre_net.p, self.decoder.prenet.p
        ec, pc = self.encoder.cbhg.dropout, self.postnet.dropout
        return dict(zip(self.SITES, (ep, ep, ec, ec, dp, dp, self.zoneout, self.zoneout, pc, pc)))

    def _draw_seeds(self) -> Dict[str, Any]:
        """one dropout_seed() per random site with p > 0, in SITES order (host integers, no device sync)"""
        forced = self._forced_seeds
        seeds = {}
        for name, p in self._site_p().items():
            if not 0.0 <= p < 1.0:
                raise FtError(f'Tacotron.forward_train: the probability of site {name} must be in [0, 1) (got {p})')
            seeds[name] = None if p <= 0.0 else (int(forced[name]) if forced is not None else dropout_seed())
        return seeds

    def forward_train(self, batch: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """models/tacotron.py:219-280 in training mode -> (mel_outputs [B,80,S*r], linear [B,80,S*r], attn_scores
        [B,S,Tx]), S = ceil(steps / r).  mel_outputs and linear carry an autograd graph whose nodes are HIP kernel
        sequences (ops.py, taco_ops.py); attn_scores is NOT differentiable (the reference's trainer only scores it,
        taco_trainer.py:100).  Needs the whole module tree in training mode and a HIP device.  As the reference's train()
        forward it adds 1 to `step` and updates every BatchNorm's running statistics and num_batches_tracked.  The ten
        random sites (eight dropouts, two zoneouts; module docstring) draw their seeds from torch's host generator;
        self.last_seeds holds them afterwards."""
        for name, m in self.named_modules():
            if not m.training:
                raise FtError(f'Tacotron.forward_train: module {name or "<root>"} is in eval mode; call model.train() '
                              '(forward / align are the inference paths)')
        w = self.encoder.embedding.weight
        if not w.is_cuda:
            raise FtError('Tacotron.forward_train runs on an MI355X (HIP) device only: move the model with .cuda()')
        x, mel, semb = self._check_batch(batch)
        seeds = self._draw_seeds()
        p = self._site_p()
        self.last_seeds = dict(seeds)
        self.step += 1
        for m in self.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.num_batches_tracked += 1
        B, Tx = x.shape
        r, steps = self.r, mel.shape[2]
        S = math.ceil(steps / r)
        enc, dec = self.encoder, self.decoder

        def prenet(pn, y, site):
            y = TO.PreNetLayerFn.apply(y, pn.fc1.weight, pn.fc1.bias, p[site + '.fc1'], seeds[site + '.fc1'])
            return TO.PreNetLayerFn.apply(y, pn.fc2.weight, pn.fc2.bias, p[site + '.fc2'], seeds[site + '.fc2'])

        y = ops.EmbeddingFn.apply(x, enc.embedding.weight)
        y = prenet(enc.pre_net, y, 'encoder.pre_net')
        e = enc.cbhg(y, seeds=(seeds['encoder.cbhg.bank'], seeds['encoder.cbhg.conv_project1']))     # [B,Tx,256]
        if semb is not None:
            e = ops.ConcatColsFn.apply(e, None, semb, B, Tx, False)
        ep = ops.LinearFn.apply(e, self.encoder_proj.weight, None)
        epq = ops.LinearFn.apply(e, self.encoder_proj_query.weight, None)
        frames = torch.empty(S, B, self.n_mels, device=x.device, dtype=torch.float32)
        _lib.call('ft_taco_frames', _p(mel), B, self.n_mels, steps, r, S, _p(frames), _stream())
        pre = prenet(dec.prenet, frames, 'decoder.prenet')                                            # [S,B,128]
        gru, lsa = dec.attn_rnn, dec.attn_net
        hist, attn = TO.TacoAttendFn.apply(ep, epq, pre, gru.weight_ih, gru.bias_ih, gru.weight_hh, gru.bias_hh,
                                           lsa.W.weight, lsa.W.bias, lsa.conv.weight, lsa.L.weight, lsa.L.bias,
                                           lsa.v.weight)
        h = ops.LinearFn.apply(hist, dec.rnn_input.weight, dec.rnn_input.bias)                        # [S,B,L]
        for cell, site in ((dec.res_rnn1, 'decoder.res_rnn1'), (dec.res_rnn2, 'decoder.res_rnn2')):
            h = TO.AddFn.apply(h, TO.ZoneoutLSTMFn.apply(h, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh,
                                                         p[site], seeds[site] or 0))
        yv = TO.MelProjFn.apply(h, dec.mel_proj.weight, self.n_mels, Decoder.max_r, r)                # [S,B,r*80]
        mel_cl = ops.BTTransposeFn.apply(yv, False).reshape(B, S * r, self.n_mels)                    # frame i*r + k
        post = self.postnet(mel_cl, time_major_out=True,
                            seeds=(seeds['postnet.bank'], seeds['postnet.conv_project1']))            # [T,B,2*dims]
        lin = ops.LinearFn.apply(post, self.post_proj.weight, None, B)                                # [B,T,80]
        T = S * r
        return ops.TransposePadFn.apply(mel_cl, T, 0.0), ops.TransposePadFn.apply(lin, T, 0.0), attn

    def _mel_path(self, hist: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """history [S,B,512] -> (mel_outputs, linear) [B,80,S*r]"""
        S, B = hist.shape[:2]
        r = self.r
        dec = self.decoder
        h = H.linear_fwd(hist, dec.rnn_input.weight, dec.rnn_input.bias)     # [S,B,L]  rnn_input([context, h_attn])
        h = self._add(h, self._lstm(dec.res_rnn1, h))
        h = self._add(h, self._lstm(dec.res_rnn2, h))
        # mel_proj rows n * 20 + k (k < r) -- the [:, :, :r] slice of the [B, 80, 20] view -- in the order k * 80 + n,
        # so that row (i, b) of the product is frames i*r .. i*r + r-1 of item b, channels last
        n_mels, max_r = self.n_mels, Decoder.max_r
        w_mel = self._pack(('mel_proj', r), dec.mel_proj.weight,
                           lambda: H.bt_transpose(dec.mel_proj.weight.detach().reshape(n_mels, max_r, -1), True)[:r]
                           .reshape(r * n_mels, -1))
        y = H.linear_fwd(h, w_mel)                                              # [S,B,r*80]
        mel_cl = H.bt_transpose(y, False).reshape(B, S * r, n_mels)             # [B,S*r,80], frame i*r + k
        return self._post(mel_cl)

    def _post(self, mel_cl: torch.Tensor, mel_len: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """frames [B,T,80] (channels last) -> (mel_outputs, linear) [B,80,T]: the postnet CBHG and post_proj.
        mel_len (int64 [B], device; generate_batch): item b has mel_len[b] frames, the rest is masked in front of the
        postnet's convolutions and comes back as base.PAD_VALUE (as ForwardTacotron._ragged_finish)"""
        B, T = mel_cl.shape[:2]
        if mel_len is None:
            post = self.postnet(mel_cl, time_major_out=True)                    # [T,B,2*postnet_dims]
            lin = H.linear_fwd(post, self.post_proj.weight, x_tm_B=B, y_tm_B=0)     # [B,T,80]
            return H.transpose_pad_fwd(mel_cl, T, 0.0), H.transpose_pad_fwd(lin, T, 0.0)
        mel_cl = H.mask_rows(mel_cl, mel_len)
        post = self.postnet.forward_lens(mel_cl, mel_len, time_major_out=True)
        lin = H.linear_fwd(post, self.post_proj.weight, x_tm_B=B, y_tm_B=0)
        return H.transpose_pad_lens_fwd(mel_cl, mel_len, T, PAD_VALUE), H.transpose_pad_lens_fwd(lin, mel_len, T, PAD_VALUE)


def l1_loss(x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """F.l1_loss(x, target) (mean) of [B,C,T] tensors on the HIP loss kernel: ops.masked_l1 with full lengths.  The
    reference loop's loss is l1_loss(m1_hat, m) + l1_loss(m2_hat, m) (taco_trainer.py:96-98)."""
    lens = torch.full((x.shape[0],), x.shape[2], dtype=torch.int64, device=x.device)
    return ops.masked_l1(x, target, lens)
