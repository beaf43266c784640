"""MI355X-native ForwardTacotron: same constructor, batch-dict forward()/generate() and state_dict as
the reference (models/forward_tacotron.py:14-254, models/common_layers.py:12-124) -- 322 state_dict
entries with identical names / shapes / dtypes, identical default initialisation under the same seed --
but every forward and backward computation is a hand-written gfx950 kernel behind the C ABI.

torch.nn.{Embedding,Conv1d,BatchNorm1d,Linear} objects appear below ONLY as parameter containers (they
give the reference's exact names and default init); their forward() is never called.  There is no
CPU / eager fallback: the model refuses to run if its tensors are not on a HIP device.
"""
import math
import os
from typing import Callable, Dict, List, Optional

import torch
import torch.nn as nn

from . import hip as H
from . import ops
from .base import (AcousticModel, LengthRegulator, NUM_CHARS_DEFAULT, PAD_VALUE, _dropout, _seed,  # noqa: F401
                   _side_priority, predictor_front, predictor_tail)                                # (re-exported)


class _RNNParams(nn.Module):
    """Parameter container with nn.GRU / nn.LSTM (1 layer, bidirectional) names and init
    (uniform(-1/sqrt(H), 1/sqrt(H)) in registration order, like torch's RNNBase.reset_parameters)."""

    def __init__(self, input_size: int, hidden_size: int, gates: int) -> None:
        super().__init__()
        self.input_size, self.hidden_size, self.gates = input_size, hidden_size, gates
        for sfx in ('', '_reverse'):
            self.register_parameter('weight_ih_l0' + sfx, nn.Parameter(torch.empty(gates * hidden_size, input_size)))
            self.register_parameter('weight_hh_l0' + sfx, nn.Parameter(torch.empty(gates * hidden_size, hidden_size)))
            self.register_parameter('bias_ih_l0' + sfx, nn.Parameter(torch.empty(gates * hidden_size)))
            self.register_parameter('bias_hh_l0' + sfx, nn.Parameter(torch.empty(gates * hidden_size)))
        stdv = 1.0 / math.sqrt(hidden_size) if hidden_size > 0 else 0
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def weights(self) -> List[torch.Tensor]:
        return [self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0,
                self.weight_ih_l0_reverse, self.weight_hh_l0_reverse, self.bias_ih_l0_reverse,
                self.bias_hh_l0_reverse]


class GRU(_RNNParams):
    """nn.GRU(in, H, batch_first=True, bidirectional=True) replacement (common_layers.py:89)."""

    def __init__(self, input_size: int, hidden_size: int) -> None:
        super().__init__(input_size, hidden_size, 3)

    def forward(self, x: torch.Tensor, time_major_out: bool = False) -> torch.Tensor:
        """x [B,T,in] -> [B,T,2H]; time_major_out=True returns the recurrence's native [T,B,2H] layout
        (what the fused consumers inside this package read directly)."""
        y = ops.BiGRUFn.apply(x, *self.weights())
        return y if time_major_out else ops.BTTransposeFn.apply(y, False)

    def forward_lens(self, x: torch.Tensor, lens: torch.Tensor, time_major_out: bool = False) -> torch.Tensor:
        """pack_padded_sequence(x, lens) -> GRU -> pad_packed_sequence: item b runs over lens[b] steps (the reverse
        direction from lens[b] - 1) and the result is zero at t >= lens[b].  Inference only (no graph)."""
        y = ops.bigru_lens(x, lens, *self.weights())
        return y if time_major_out else ops.BTTransposeFn.apply(y, False)


class LSTM(_RNNParams):
    """nn.LSTM(in, H, batch_first=True, bidirectional=True) replacement with the pack/unpack semantics of
    forward_tacotron.py:147-152 built in (lens + padding_value)."""

    def __init__(self, input_size: int, hidden_size: int) -> None:
        super().__init__(input_size, hidden_size, 4)

    def forward(self, x: torch.Tensor, lens: Optional[torch.Tensor], pad_value: float) -> torch.Tensor:
        return ops.BiLSTMFn.apply(x, lens, pad_value, *self.weights())

    def forward_regulated(self, x: torch.Tensor, dur: torch.Tensor, lens: Optional[torch.Tensor],
                          pad_value: float) -> torch.Tensor:
        """self(LengthRegulator()(x, dur, lens), lens, pad_value) as one node, with the input projection formed per
        token instead of per frame (ops.LRBiLSTMFn); x is the token-level input [B,Tx,I]"""
        if not dur.is_contiguous() or dur.dtype != torch.float32:
            raise H._lib.FtError('LengthRegulator: dur must be contiguous fp32 (it is clamped in place)')
        return ops.LRBiLSTMFn.apply(x, dur, lens, pad_value, *self.weights())


def regulate_and_decode(model, x: torch.Tensor, dur: torch.Tensor, mel_lens: Optional[torch.Tensor]) -> torch.Tensor:
    """LengthRegulator + decoder LSTM of the ForwardTacotron variants (forward_tacotron.py:145-152), and the place where
    trainer.TrainStep's staged backward cuts the graph.  FT_LR_LSTM_FUSED=0 keeps the two as separate nodes."""
    staged = model.training and torch.is_grad_enabled() and model.stage_backward
    fused = os.environ.get('FT_LR_LSTM_FUSED', '1') != '0'
    if not fused:
        x = model.lr(x, dur, mel_lens)      # at max(mel_lens) frames, the length pad_packed_sequence returns (:147-152)
    if staged:
        # trainer.TrainStep runs the backward in three stages (postnet .. LSTM | predictors | LR .. prenet): the graph is
        # cut here, below the (regulated) LSTM, and the trainer feeds the cut's gradient into the lower part itself
        cut = x.detach().requires_grad_(True)
        model._cut = (x, cut)
        x = cut
    if fused:
        return model.lstm.forward_regulated(x, dur, mel_lens, model.padding_value)
    return model.lstm(x, mel_lens, model.padding_value)


class HighwayNetwork(nn.Module):
    """common_layers.py:27-40"""

    def __init__(self, size: int) -> None:
        super().__init__()
        self.W1 = nn.Linear(size, size)
        self.W2 = nn.Linear(size, size)
        self.W1.bias.data.fill_(0.)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.HighwayFn.apply(x, self.W1.weight, self.W1.bias, self.W2.weight, self.W2.bias)


class BatchNormConv(nn.Module):
    """common_layers.py:43-57 on channels-last input; conv -> ReLU -> BatchNorm (+ residual)."""

    def __init__(self, in_channels: int, out_channels: int, kernel: int, relu=True) -> None:
        super().__init__()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel, stride=1, padding=kernel // 2, bias=False)
        self.bnorm = nn.BatchNorm1d(out_channels)
        self.relu = relu

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        bn = self.bnorm
        if self.training:
            return ops.BatchNormConvFn.apply(x, self.conv.weight, bn.weight, bn.bias, residual, bn.running_mean,
                                             bn.running_var, self.relu is True)
        return self._eval(x, residual)

    def forward_lens(self, x: torch.Tensor, lens: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """eval forward of a ragged batch whose rows t >= lens[b] are zero on input: they are stored as zeros again
        (scale * relu(conv) + shift is not zero there), so the next convolution reads zeros across an item's end"""
        if self.training:
            raise H._lib.FtError('BatchNormConv.forward_lens is the eval-mode (inference) path')
        return self._eval(x, residual, lens)

    def _eval(self, x: torch.Tensor, residual: Optional[torch.Tensor], lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """eval: BatchNorm folds into the conv epilogue (scale/shift after the ReLU); lens: the ragged-batch form"""
        bn = self.bnorm
        _eval_needs_no_grad(x, self.conv.weight)
        scale, shift = H.bn_fold_eval(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        wp = H.conv_pack_weight(self.conv.weight)
        acc = _c_clone(residual) if residual is not None else None
        if lens is None:
            return H.conv1d_fwd(x.contiguous(), wp, relu=self.relu is True, Tout=x.shape[1], scale=scale, shift=shift,
                                accumulate_into=acc)
        return H.conv1d_fwd_lens(x.contiguous(), wp, relu=self.relu is True, lens=lens, scale=scale, shift=shift,
                                 accumulate_into=acc)


def _eval_needs_no_grad(x: torch.Tensor, w: torch.Tensor) -> None:
    """The eval-mode BatchNormConv / conv-bank path is raw kernel launches (BatchNorm folded into the convolution's
    epilogue): it records no autograd graph.  The reference's eval forward IS differentiable; rather than hand back
    tensors that silently carry no gradient, refuse the combination (the reference's own eval call sites --
    evaluate(), generate(), create_gta_features -- all run under torch.no_grad())."""
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        raise H._lib.FtError('eval-mode forward is not differentiable here (BatchNorm is folded into the convolution '
                             'epilogue): call it under torch.no_grad(), or use model.train() for gradients')


def _c_clone(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().clone()


class CBHG(nn.Module):
    """common_layers.py:60-124 on channels-last tensors: x [B,T,in] -> [B,T,2*channels]."""

    def __init__(self, K: int, in_channels: int, channels: int, proj_channels: list, num_highways: int,
                 dropout: float = 0.5) -> None:
        super().__init__()
        self.dropout = dropout
        self.bank_kernels = [i for i in range(1, K + 1)]
        self.conv1d_bank = nn.ModuleList()
        for k in self.bank_kernels:
            self.conv1d_bank.append(BatchNormConv(in_channels, channels, k))
        self.conv_project1 = BatchNormConv(len(self.bank_kernels) * channels, proj_channels[0], 3)
        self.conv_project2 = BatchNormConv(proj_channels[0], proj_channels[1], 3, relu=False)
        self.pre_highway = nn.Linear(proj_channels[-1], channels, bias=False)
        self.highways = nn.ModuleList()
        for _ in range(num_highways):
            self.highways.append(HighwayNetwork(channels))
        self.rnn = GRU(channels, channels)
        self._flat = None

    # -- the K BatchNorms of the bank share flat storage so one kernel normalises the whole [B,T,K*C] buffer
    def _bank_flat(self):
        """Returns flat [K*C] aliases (gamma, beta, running_mean, running_var) of the members' tensors.
        Members already adjacent in memory (e.g. placed so by parallel.FlatParams, or by an earlier call)
        are aliased as they are; otherwise they are re-homed into one fresh buffer.  load_state_dict copies
        in place and keeps the aliasing; .to()/.cuda() break it and are repaired here."""
        bns = [m.bnorm for m in self.conv1d_bank]
        K, C = len(bns), bns[0].weight.numel()
        out = []
        for name in ('weight', 'bias', 'running_mean', 'running_var'):
            ts = [getattr(b, name) for b in bns]
            base = ts[0].data_ptr()
            adjacent = all(ts[i].data_ptr() == base + 4 * i * C for i in range(1, K)) and \
                ts[0].untyped_storage().nbytes() - 4 * ts[0].storage_offset() >= 4 * K * C
            if not adjacent:
                flat = torch.cat([t.detach().reshape(-1) for t in ts]).contiguous()
                for i, b in enumerate(bns):
                    view = flat[i * C:(i + 1) * C]
                    if name in ('weight', 'bias'):
                        getattr(b, name).data = view
                    else:
                        b._buffers[name] = view
                ts = [getattr(b, name) for b in bns]
            out.append(ts[0].detach().as_strided((K * C,), (1,)))
        return out

    def _site(self, y: torch.Tensor, seeds, i: int) -> torch.Tensor:
        """dropout site i (0: behind the pooled bank, 1: behind conv_project1); seeds: None = draw from base._seed(), else
        the caller's pair of seeds, a None entry skipping its site (Tacotron.forward_train records what it passes)"""
        if seeds is None:
            return _dropout(y, self.dropout, self.training)
        return y if seeds[i] is None else ops.DropoutFn.apply(y, self.dropout, seeds[i])

    def forward(self, x: torch.Tensor, time_major_out: bool = False, seeds=None) -> torch.Tensor:
        if not self.training:
            return self._eval(x, time_major_out)
        K = len(self.bank_kernels)
        gamma, beta, rm, rv = self._bank_flat()
        ws = [m.conv.weight for m in self.conv1d_bank]
        gs = [m.bnorm.weight for m in self.conv1d_bank]
        bs = [m.bnorm.bias for m in self.conv1d_bank]
        y = ops.ConvBankFn.apply(x, K, gamma, beta, rm, rv, *ws, *gs, *bs)
        y = self._site(y, seeds, 0)
        y = self.conv_project1(y)
        y = self._site(y, seeds, 1)
        y = self.conv_project2(y, residual=x)
        y = ops.LinearFn.apply(y, self.pre_highway.weight, None)
        y = ops.highway_stack(y, list(self.highways))     # gates inside the GEMM epilogues (width % 32 == 0)
        return self.rnn(y, time_major_out=time_major_out)

    def forward_lens(self, x: torch.Tensor, lens: torch.Tensor, time_major_out: bool = False) -> torch.Tensor:
        """eval forward of a ragged batch: x [B,T,in] is zero at t >= lens[b] and so is the result; every valid row
        is what the item gets alone at T = lens[b] (where each mask sits).  The bank's own store
        needs no mask: its only reader across time is the max-pool, which masks its output."""
        if self.training:
            raise H._lib.FtError('CBHG.forward_lens is the eval-mode (inference) path')
        return self._eval(x, time_major_out, lens)

    def _eval(self, x: torch.Tensor, time_major_out: bool, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """eval: the bank's BatchNorms fold into its convolutions' epilogue; lens: the ragged-batch form of every step
        that reads across time"""
        K = len(self.bank_kernels)
        C = self.conv1d_bank[0].conv.weight.shape[0]
        gamma, beta, rm, rv = self._bank_flat()
        T = x.shape[1]
        _eval_needs_no_grad(x, self.conv1d_bank[0].conv.weight)
        scale, shift = H.bn_fold_eval(gamma, beta, rm, rv, self.conv1d_bank[0].bnorm.eps)
        wp_all = torch.cat([H.conv_pack_weight(m.conv.weight).reshape(-1) for m in self.conv1d_bank])
        y = H.conv_bank_fwd(x, wp_all, K, C, relu=True, Tout=T, scale=scale, shift=shift)
        y = H.maxpool2_fwd(y) if lens is None else H.maxpool2_fwd_lens(y, lens)
        y = self.conv_project1._eval(y, None, lens)
        y = self.conv_project2._eval(y, x, lens)
        y = ops.LinearFn.apply(y, self.pre_highway.weight, None)
        y = ops.highway_stack(y, list(self.highways))     # gates inside the GEMM epilogues (width % 32 == 0)
        if lens is None:
            return self.rnn(y, time_major_out=time_major_out)
        return self.rnn.forward_lens(y, lens, time_major_out=time_major_out)


class SeriesPredictor(nn.Module):
    """forward_tacotron.py:14-39 ; returns [B,T,1]."""

    def __init__(self, num_chars, emb_dim=64, conv_dims=256, rnn_dims=64, dropout=0.5):
        super().__init__()
        self.embedding = nn.Embedding(num_chars, emb_dim)
        self.convs = nn.ModuleList([
            BatchNormConv(emb_dim, conv_dims, 5, relu=True),
            BatchNormConv(conv_dims, conv_dims, 5, relu=True),
            BatchNormConv(conv_dims, conv_dims, 5, relu=True),
        ])
        self.rnn = GRU(conv_dims, rnn_dims)
        self.lin = nn.Linear(2 * rnn_dims, 1)
        self.dropout = dropout

    def forward(self, x: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
        return conv_gru_predict(self, predictor_front(x, self.embedding), alpha)

    def forward_lens(self, x: torch.Tensor, lens: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
        """eval forward of a ragged batch: tokens at t >= lens[b] are ignored, the result [B,T,1] is zero there"""
        B = x.shape[0]
        y = H.embedding_fwd_lens(x, lens, self.embedding.weight)             # the pad id has a learned embedding
        for conv in self.convs:
            y = conv.forward_lens(y, lens)
        y = self.rnn.forward_lens(y, lens, time_major_out=True)
        return H.mask_rows(predictor_tail(y, self.lin, alpha, B), lens)      # (the Linear's bias)


def conv_gru_predict(pred: nn.Module, x: torch.Tensor, alpha: float) -> torch.Tensor:
    """3 x (BatchNormConv, dropout) -> biGRU -> Linear (/ alpha) of the conv-GRU series predictors, on the output of
    base.predictor_front"""
    for conv in pred.convs:
        x = conv(x)
        x = _dropout(x, pred.dropout, pred.training)
    B = x.shape[0]
    x = pred.rnn(x, time_major_out=True)
    return predictor_tail(x, pred.lin, alpha, B)                           # [T,B,2H] -> [B,T,out]


class ForwardTacotron(AcousticModel):
    """Drop-in for models/forward_tacotron.py:42-254."""
    config_key = 'forward_tacotron'
    recurrent = True

    def __init__(self,
                 embed_dims: int, series_embed_dims: int, num_chars: int,
                 durpred_conv_dims: int, durpred_rnn_dims: int, durpred_dropout: float,
                 pitch_conv_dims: int, pitch_rnn_dims: int, pitch_dropout: float, pitch_strength: float,
                 energy_conv_dims: int, energy_rnn_dims: int, energy_dropout: float, energy_strength: float,
                 rnn_dims: int, prenet_dims: int, prenet_k: int, postnet_num_highways: int,
                 prenet_dropout: float, postnet_dims: int, postnet_k: int, prenet_num_highways: int,
                 postnet_dropout: float, n_mels: int, padding_value=PAD_VALUE):
        super().__init__()
        self._ctor_kwargs = {k: v for k, v in locals().items() if k not in ('self', '__class__')}
        self.rnn_dims = rnn_dims
        self.padding_value = padding_value
        self.embedding = nn.Embedding(num_chars, embed_dims)
        self.lr = LengthRegulator()
        self.dur_pred = SeriesPredictor(num_chars=num_chars, emb_dim=series_embed_dims,
                                        conv_dims=durpred_conv_dims, rnn_dims=durpred_rnn_dims,
                                        dropout=durpred_dropout)
        self.pitch_pred = SeriesPredictor(num_chars=num_chars, emb_dim=series_embed_dims,
                                          conv_dims=pitch_conv_dims, rnn_dims=pitch_rnn_dims,
                                          dropout=pitch_dropout)
        self.energy_pred = SeriesPredictor(num_chars=num_chars, emb_dim=series_embed_dims,
                                           conv_dims=energy_conv_dims, rnn_dims=energy_rnn_dims,
                                           dropout=energy_dropout)
        self.prenet = CBHG(K=prenet_k, in_channels=embed_dims, channels=prenet_dims,
                           proj_channels=[prenet_dims, embed_dims], num_highways=prenet_num_highways,
                           dropout=prenet_dropout)
        self.lstm = LSTM(2 * prenet_dims, rnn_dims)
        self.lin = nn.Linear(2 * rnn_dims, n_mels)
        self.register_buffer('step', torch.zeros(1, dtype=torch.long))
        self.postnet = CBHG(K=postnet_k, in_channels=n_mels, channels=postnet_dims,
                            proj_channels=[postnet_dims, n_mels], num_highways=postnet_num_highways,
                            dropout=postnet_dropout)
        self.post_proj = nn.Linear(2 * postnet_dims, n_mels, bias=False)
        self.pitch_strength = pitch_strength
        self.energy_strength = energy_strength
        self.pitch_proj = nn.Conv1d(1, 2 * prenet_dims, kernel_size=3, padding=1)
        self.energy_proj = nn.Conv1d(1, 2 * prenet_dims, kernel_size=3, padding=1)

    def _trunk(self, x: torch.Tensor, dur, pitch, energy, mel_lens: Optional[torch.Tensor], late_inputs=None):
        """late_inputs (inference): a callable that delivers (dur, pitch, energy) once the prenet has been enqueued -- the
        predictors then run on a side stream beside embedding + prenet CBHG instead of in front of them"""
        B = x.shape[0]
        x = ops.EmbeddingFn.apply(x, self.embedding.weight)
        x = self.prenet(x, time_major_out=True)                             # [Tx,B,2P] (recurrence layout)
        if late_inputs is not None:
            dur, pitch, energy = late_inputs()
        x = self._cond_add(x, pitch, energy, True)                          # -> [B,Tx,2P]
        x = regulate_and_decode(self, x, dur, mel_lens)
        mel = ops.LinearFn.apply(x, self.lin.weight, self.lin.bias)        # [B,T,n_mels]
        post = self.postnet(mel, time_major_out=True)                       # [T,B,2Q]
        post = ops.LinearFn.apply(post, self.post_proj.weight, None, B)     # -> [B,T,n_mels]
        return mel, post

    def _predict(self, x: torch.Tensor, alpha: float = 1.0, pitch_function=lambda p: p, energy_function=lambda e: e):
        """the three predictors, in the order that fixes the dropout seed sequence: dur, pitch, energy"""
        dur_hat = self.dur_pred(x, alpha=alpha).squeeze(-1)
        pitch_hat = pitch_function(self.pitch_pred(x).transpose(1, 2))
        energy_hat = energy_function(self.energy_pred(x).transpose(1, 2))
        return {'dur': dur_hat, 'pitch': pitch_hat, 'energy': energy_hat}

    def forward(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        x = batch['x']
        mel = batch['mel']
        dur = batch['dur']
        mel_lens = batch['mel_len']
        pitch = batch['pitch']               # [B,Tx]  (the reference unsqueezes to [B,1,Tx] for its Conv1d)
        energy = batch['energy']
        self._begin_forward(x)

        # The three predictors are independent of the trunk (forward_tacotron.py:129-131 vs :133-159) and
        # their 128-step recurrences are latency-bound, so they run on a side HIP stream concurrently with the
        # trunk; autograd replays each backward node on the stream of its forward, so the overlap also holds
        # in backward.
        fork = self._fork_predictors(x.device, lambda: self._predict(x))
        mel_cl, post_cl = self._trunk(x, dur, pitch, energy, mel_lens.to(device=x.device, dtype=torch.long))
        Tout = mel.size(2)
        x_post = ops.TransposePadFn.apply(post_cl, Tout, self.padding_value)
        x_mel = ops.TransposePadFn.apply(mel_cl, Tout, self.padding_value)
        return {'mel': x_mel, 'mel_post': x_post, **self._join_predictors(fork)}

    def generate(self, x: torch.Tensor, alpha=1.0,
                 pitch_function: Callable[[torch.Tensor], torch.Tensor] = lambda x: x,
                 energy_function: Callable[[torch.Tensor], torch.Tensor] = lambda x: x) -> Dict[str, torch.Tensor]:
        self.eval()
        with torch.no_grad():
            return self._generate(x, alpha, pitch_function, energy_function)

    def generate_jit(self, x: torch.Tensor, alpha: float = 1.0, beta: float = 1.0) -> Dict[str, torch.Tensor]:
        """forward_tacotron.py:186-200: generate with the pitch scaled by beta.  Eager entry; the TorchScript surface
        (`torch.jit.script(model).generate_jit`, README.md:159-171 of the reference) is export.ScriptedForwardTacotron,
        which reaches this same path through the opaque operator torch.ops.fwdtaco.generate_jit."""
        with torch.no_grad():
            return self._generate(x, alpha, lambda p: ops.ScaleFn.apply(p, beta) if beta != 1.0 else p, lambda e: e)

    def __prepare_scriptable__(self):
        """torch.jit.script(model) compiles the flat-buffer twin (export.py), not this kernel-launching module tree."""
        from . import export
        return export.scriptable(self, self._ctor_kwargs)

    def _generate(self, x, alpha, pitch_function, energy_function):
        self._require_device(x)
        # forward_tacotron.py:168-189 runs the predictors first, then the prenet; here they run beside it
        pred, late_inputs = self._generate_fork(x, lambda: self._predict(x, alpha, pitch_function, energy_function))
        mel_cl, post_cl = self._trunk(x, None, None, None, None, late_inputs=late_inputs)
        T = mel_cl.shape[1]
        return {'mel': H.transpose_pad_fwd(mel_cl, T, 0.0), 'mel_post': H.transpose_pad_fwd(post_cl, T, 0.0), **pred}

    # -- generate_batch: what base.AcousticModel's driver needs from this model -----------------------------------
    def _ragged_prenet(self, x, xl):
        h = H.embedding_fwd_lens(x, xl, self.embedding.weight)
        return self.prenet.forward_lens(h, xl, time_major_out=True)           # [Tx,B,2P], zero at t >= x_len[b]

    def _ragged_regulate(self, h, pred):
        h = self._cond_add(h, pred['pitch'], pred['energy'], True)            # -> [B,Tx,2P]
        return regulate_and_decode(self, h, pred['dur'], pred['mel_len'])     # packed LSTM; syncs to size Tm

    def _ragged_finish(self, h, mel_len):
        B = h.shape[0]
        # lin's bias (and the LSTM's padding_value) make the padded frames non-zero: mask before the postnet's convolutions
        mel = H.mask_rows(ops.LinearFn.apply(h, self.lin.weight, self.lin.bias), mel_len)
        post = self.postnet.forward_lens(mel, mel_len, time_major_out=True)  # [Tm,B,2Q]
        post = ops.LinearFn.apply(post, self.post_proj.weight, None, B)      # -> [B,Tm,n_mels]
        Tm = mel.shape[1]
        pad = float(self.padding_value)
        return H.transpose_pad_lens_fwd(mel, mel_len, Tm, pad), H.transpose_pad_lens_fwd(post.contiguous(), mel_len, Tm, pad)

    def _generate_mel(self, x: torch.Tensor, dur_hat: torch.Tensor, pitch_hat: torch.Tensor,
                      energy_hat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """forward_tacotron.py:205-234: mel generation from given durations [B,Tx], pitch and energy [B,1,Tx]; the LSTM
        runs over the padded length (no packing).  `dur_hat` is clamped in place like every LengthRegulator input."""
        self._require_device(x)
        dur_in = dur_hat.contiguous()
        mel_cl, post_cl = self._trunk(x, dur_in, pitch_hat.reshape(x.shape[0], -1).contiguous(),
                                      energy_hat.reshape(x.shape[0], -1).contiguous(), None)
        T = mel_cl.shape[1]
        return {'mel': H.transpose_pad_fwd(mel_cl, T, 0.0), 'mel_post': H.transpose_pad_fwd(post_cl, T, 0.0),
                'dur': dur_in, 'pitch': pitch_hat, 'energy': energy_hat}


from . import export as _export  # noqa: E402,F401  (registers torch.ops.fwdtaco.generate_jit for torch.jit.load)
