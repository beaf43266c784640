"""What the four acoustic models (ForwardTacotron, MultiForwardTacotron, FastPitch, MultiFastPitch) share: the
dependency-free helpers, the predictors' common front and tail, and AcousticModel -- the base class that carries the
host-side plumbing (device check, predictor side stream and its fork / join, step counters, config / checkpoint
constructors) and documents what trainer.TrainStep and parallel.FlatBuffers expect of a model.
"""
import os
from pathlib import Path
from typing import Any, Callable, Dict, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import hip as H
from . import ops

PAD_VALUE = -11.5129
NUM_CHARS_DEFAULT = 135      # len(utils.text.symbols.phonemes), utils/text/symbols.py:21-23


_seed_state = {'torch_seed': None, 'base': 0, 'n': 0}


def _seed() -> int:
    """Seed of one dropout site: host arithmetic only (no device sync, no tensor op -- a step draws ~170 of them).
    The stream is re-based from torch's host RNG whenever torch.manual_seed() installs a different seed."""
    st = _seed_state
    s = torch.initial_seed()
    if st['torch_seed'] != s:
        st['torch_seed'] = s
        st['base'] = int(torch.randint(0, 2 ** 62, (1,)).item())
        st['n'] = 0
    st['n'] += 1
    return (st['base'] + 0x9E3779B97F4A7C15 * st['n']) & ((1 << 62) - 1)


def _side_priority() -> int:
    return -1 if os.environ.get('FT_PRED_PRIORITY', '1') == '1' else 0


def _gen_overlap() -> bool:
    """inference runs the predictors on the side stream, beside the prenet; FT_GEN_OVERLAP=0: in front of it"""
    return os.environ.get('FT_GEN_OVERLAP', '1') == '1'


def _dropout(x: torch.Tensor, p: float, training: bool) -> torch.Tensor:
    if not training or p <= 0.0:
        return x
    return ops.DropoutFn.apply(x, p, _seed())


class LengthRegulator(nn.Module):
    """common_layers.py:12-24"""

    def forward(self, x: torch.Tensor, dur: torch.Tensor, pack_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """pack_lens: lengths the result will be packed with (see ops.LengthRegulateFn); None = reference signature"""
        if not dur.is_contiguous() or dur.dtype != torch.float32:
            raise H._lib.FtError('LengthRegulator: dur must be contiguous fp32 (it is clamped in place)')
        return ops.LengthRegulateFn.apply(x, dur, pack_lens)


def predictor_front(x: torch.Tensor, embedding: nn.Embedding, x_cond: Optional[torch.Tensor] = None,
                    cond_embedding: Optional[nn.Embedding] = None,
                    speaker_emb: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What every series predictor starts with: token embedding ++ conditional embedding ++ speaker embedding repeated
    over time (the last two optional) -> [B,T,C]"""
    B, T = x.shape
    e = ops.EmbeddingFn.apply(x, embedding.weight)
    if x_cond is None and speaker_emb is None:
        return e
    c = ops.EmbeddingFn.apply(x_cond, cond_embedding.weight) if x_cond is not None else None
    return ops.ConcatColsFn.apply(e, c, speaker_emb, B, T, False)


def predictor_tail(x: torch.Tensor, lin: nn.Linear, alpha: float, x_tm_B: int = 0) -> torch.Tensor:
    """What every series predictor ends with: Linear, then / alpha -> [B,T,out]; x_tm_B > 0: x is a time-major
    [T,B,C] recurrence output (ops.LinearFn)"""
    x = ops.LinearFn.apply(x, lin.weight, lin.bias, x_tm_B)
    if alpha != 1.0:
        x = ops.ScaleFn.apply(x, 1.0 / alpha)
    return x


class AcousticModel(nn.Module):
    """Base of the four acoustic models.  It registers no parameter, buffer or submodule: every subclass builds its
    modules and its `step` buffer itself, in the reference's order (which fixes the state_dict key order and the
    constructor's RNG draws).  A subclass sets `config_key` and `recurrent`, has an `embedding`, a `padding_value` and
    a `step` buffer, and runs its predictors through _fork_predictors / _join_predictors.

    The attributes below are the contract with trainer.TrainStep (which reads and sets them directly) and
    parallel.FlatBuffers; the values here are the defaults of a model that does not care."""

    config_key: str = ''            # the model's section of a config: config[config_key]['model']
    recurrent: bool = False         # the trunk has recurrences and BatchNorms (the two Tacotron variants)

    # 'fp32' (the reference's arithmetic; parity bars) or 'bf16' (BASELINE configs[2]; the FastPitch variants): matmul
    # operands rounded to bf16, fp32 accumulation; LayerNorm / softmax statistics / losses / optimizer stay fp32.
    # forward() / generate() of the FastPitch variants run under it; TrainStep extends it over backward.
    matmul_dtype: str = 'fp32'
    # predictor branches share no graph node with the trunk in training: TrainStep may run their backward as a stage of
    # its own (or, through predictor_hook, inside the forward)
    independent_predictors: bool = True
    # token-side row count (incl. the conv bank's extra row), set per forward by the recurrent models: TrainStep keeps
    # weight gradients of operands this short on the main stream (gradsink.Policy.inline_rows)
    wgrad_inline_rows: int = 0
    wgrad_defer: bool = False       # recurrences ahead (gradsink.Policy.defer); set per forward by the recurrent models
    # set by TrainStep around one forward: cut the graph below the decoder LSTM (model.regulate_and_decode), which
    # leaves (tensor below the cut, its detached twin above it) in _cut for the trainer's three-stage backward
    stage_backward: bool = False
    _cut: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
    # set by TrainStep around one forward: called with the predictors' outputs on their stream, right behind their
    # forward (the predictors' losses + backward)
    predictor_hook: Optional[Callable[[Dict[str, torch.Tensor]], None]] = None
    # flat int64 storage of every BatchNorm's num_batches_tracked (_bump_batchnorm_counters); parallel.FlatBuffers
    # points it at its own flat buffer
    _nbt_flat: Optional[torch.Tensor] = None

    def __repr__(self):
        return f'{type(self).__name__}, num params: {sum(p.numel() for p in self.parameters())}'

    def _require_device(self, t: torch.Tensor) -> None:
        if not t.is_cuda or not self.embedding.weight.is_cuda:
            raise H._lib.FtError(f'forwardtacotron_amd.{type(self).__name__} runs on an MI355X (HIP) device only: '
                                 'move the model and the batch with .cuda(); there is no CPU fallback')

    def _bump_batchnorm_counters(self) -> None:
        """num_batches_tracked += 1 for every BatchNorm1d, as one op on shared int64 storage."""
        bns = [m for m in self.modules() if isinstance(m, nn.BatchNorm1d)]
        f = self._nbt_flat
        ok = f is not None and f.device == bns[0].num_batches_tracked.device
        if ok:
            for i in (0, len(bns) - 1):
                ok = ok and bns[i].num_batches_tracked.data_ptr() == f.data_ptr() + 8 * i
        if not ok:
            f = torch.stack([b.num_batches_tracked.detach().reshape(()) for b in bns]).contiguous()
            for i, b in enumerate(bns):
                b._buffers['num_batches_tracked'] = f[i]
            self._nbt_flat = f
        f += 1

    def _begin_forward(self, x: torch.Tensor) -> None:
        """head of every forward(): device check, the trainer's weight-gradient hints, the training counters"""
        self._require_device(x)
        if self.recurrent:
            self.wgrad_inline_rows = x.shape[0] * (x.shape[1] + 1)
            self.wgrad_defer = True
        if self.training:
            self.step += 1
            if self.recurrent:          # the models with BatchNorms
                self._bump_batchnorm_counters()

    # -- the predictors' side stream ------------------------------------------------------------------------------
    def _side_stream(self, device) -> 'torch.cuda.Stream':
        key = torch.device(device).index or 0
        if not hasattr(self, '_streams'):
            self._streams = {}
        if key not in self._streams:
            # high priority like the trainer's main stream: the predictors' kernels are small and many, behind the trunk's
            # 1000-workgroup GEMMs in a default-priority queue each of them waits for a free CU (0.25 ms of the step)
            self._streams[key] = torch.cuda.Stream(device=device, priority=_side_priority())
        return self._streams[key]

    def _fork_predictors(self, device, run: Callable[[], Dict[str, torch.Tensor]], overlap: bool = True):
        """Runs the predictors (`run` -> their output dict) on the side stream, behind everything the current stream has
        been given so far, then predictor_hook on the same stream.  overlap=False: on the current stream itself.
        -> (main, side, outputs) for _join_predictors"""
        main = torch.cuda.current_stream()
        side = self._side_stream(device) if overlap else main
        side.wait_stream(main)
        with torch.cuda.stream(side):
            pred = run()
            if self.predictor_hook is not None:
                self.predictor_hook(pred)
        return main, side, pred

    def _join_predictors(self, fork) -> Dict[str, torch.Tensor]:
        """the fork's main stream waits for the predictors and takes their outputs over"""
        main, side, pred = fork
        main.wait_stream(side)
        if self.recurrent:
            H.rnn_note_join(main, side)
        for t in pred.values():
            t.record_stream(main)
        return pred

    def _generate_fork(self, x: torch.Tensor, run: Callable[[], Dict[str, torch.Tensor]]):
        """generate() of the recurrent models: the predictors only meet the trunk behind the prenet, so they run on the
        side stream while the main stream does embedding + prenet CBHG (its 128-step GRU is latency-bound: a single
        utterance spends 84 % of its time in recurrences), joined where their outputs are needed.  FT_GEN_OVERLAP=0: no
        overlap.  -> (outputs, late_inputs for _trunk); after the trunk outputs['dur'] is the tensor the trunk consumed"""
        fork = self._fork_predictors(x.device, run, overlap=_gen_overlap())
        pred, B = fork[2], x.shape[0]

        def late_inputs():
            self._join_predictors(fork)
            if torch.sum(pred['dur'].long()) <= 0:
                torch.fill_(pred['dur'], value=2.)
            pred['dur'] = pred['dur'].contiguous()
            return pred['dur'], pred['pitch'].reshape(B, -1).contiguous(), pred['energy'].reshape(B, -1).contiguous()

        return pred, late_inputs

    # -- generate_batch: the driver, its helpers and the hooks a model supplies --------------------------------------
    checks_tokens: bool = False     # token id 0 at t < x_len[b] raises (the models whose generate() masks keys where x == 0)
    speaker_emb_dims: int = 0       # > 0: the model is speaker-conditioned, generate_batch takes one speaker row per item

    def generate_batch(self, x: torch.Tensor, x_len: torch.Tensor, alpha=1.0,
                       pitch_function: Callable[[torch.Tensor], torch.Tensor] = lambda p: p,
                       energy_function: Callable[[torch.Tensor], torch.Tensor] = lambda e: e, *,
                       speaker_emb: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """generate() of a RAGGED batch of sentences: for every item b the valid parts of the result equal
        generate(x[b:b+1, :x_len[b]], alpha, ...) on the same model (to the rounding of the matmul mode; `mel_len` exactly
        in fp32 mode).

        x: int64 [B,Tx] on the device; entries at t >= x_len[b] are ignored, whatever they hold.  x_len: int64 [B], on the
        host or the device, 1 <= x_len[b] <= Tx (anything else raises FtError).  pitch_function / energy_function get
        [B,1,Tx] (zero at t >= x_len[b]) and must act PER TOKEN -- a function that mixes tokens or items (a mean over
        the batch, a filter along t) breaks the per-item contract; their results are masked again.

        A model with `checks_tokens` (FastPitch) wants valid tokens NON-ZERO.  Its generate() masks the prenet's keys where
        x == 0 (fast_pitch.py:199), which inside a sentence only happens if the pad symbol itself is used as a token; here
        the lengths say what is padding, and a 0 at t < x_len[b] raises FtError instead of being silently treated either way.

        The speaker-conditioned models (`speaker_emb_dims` > 0; their own generate_batch(x, x_len, speaker_emb, alpha, ...)
        mirrors generate(x, speaker_emb, alpha, ...)) take `speaker_emb`: float32 [B, speaker_emb_dims] on the device, ONE
        ROW PER ITEM, rows may all differ; any other shape, dtype or device raises FtError.  The contract reads
        generate(x[b:b+1, :x_len[b]], speaker_emb[b:b+1], alpha, ...) for every item with x_len[b] >= 2; `pitch_cond`
        matches exactly in fp32 mode, like `mel_len`.  Their generate() raises on a ONE-token sentence, like the reference's
        (its argmax chain squeezes the time axis away); generate_batch gives such an item the per-token result: the argmax
        over the classes for that one token, everything else as for longer items.  The result then also holds
        `pitch_cond`, int64 [B,Tx]: the per-token argmax of the pitch_cond predictor's logits at t < x_len[b], 0 past it.
        It is decided per item and token on the device and feeds the conditional embedding of that item's dur and pitch
        predictors.

        -> mel, mel_post [B,n_mels,Tm] with Tm = max(mel_len) and padding_value at t >= mel_len[b] (one tensor where the
        model's generate() returns one); mel_len int64 [B]; dur [B,Tx], pitch / energy [B,1,Tx], all three 0 at
        t >= x_len[b].  Per item: if the truncated durations of the valid tokens sum to <= 0 they all become 2.0
        (forward_tacotron.py:176-177, fast_pitch.py:176-177); repeats are (clamp(dur, 0) + 0.5).long().  One host
        synchronisation (sizing Tm), as in generate().

        The zero-token check and the range check of an x_len that lives on the device run on the device: the FtError is
        raised only after the trunk up to the regulator has been enqueued (behind that one synchronisation), and the flag
        travels through ONE pinned host word kept on the module -- so a model must not run such a call from two threads or
        on two streams at once (without `checks_tokens` a host-side x_len is checked up front and has no such limit).

        A model plugs in through three hooks, run in this order:
          _ragged_prenet(x, xl) -> h            token-side trunk up to where the predictors are needed
          _ragged_regulate(h, pred) -> h        behind the join: CondAddFn (_cond_add), then the step that synchronises
          _ragged_finish(h, mel_len) -> (mel, mel_post)   behind the flag check, up to H.transpose_pad_lens_fwd
        and overrides _ragged_predict if its predictors take more than (x, lens).  A speaker-conditioned model's
        _ragged_prenet, _ragged_regulate and _ragged_predict get the speaker rows as the keyword `semb`; the other models
        are called exactly as before."""
        if not hasattr(self, '_ragged_prenet'):
            raise H._lib.FtError(f'{type(self).__name__} has no generate_batch: it supplies no _ragged_* hooks')
        self.eval()
        with torch.no_grad():
            on_host = self._check_ragged_batch(x, x_len)
            kw = self._check_speaker_rows(x, speaker_emb)
            x = x.contiguous()
            xl = x_len.to(x.device).contiguous()
            # the predictors only meet the trunk behind the prenet: side stream, as in _generate_fork
            fork = self._fork_predictors(x.device, lambda: self._ragged_predict(x, xl, alpha, pitch_function, energy_function,
                                                                                **kw), overlap=_gen_overlap())
            h = self._ragged_prenet(x, xl, **kw)
            pred = self._join_predictors(fork)
            # a host-side x_len was range-checked up front; what was not rides on the one synchronisation of the regulator
            read_flag = (not on_host) or self.checks_tokens
            if read_flag:
                bad_host = self._bad_flag_host()
                bad_host.copy_(pred['bad'], non_blocking=True)
            h = self._ragged_regulate(h, pred, **kw)
            flags = int(bad_host[0]) if read_flag else 0
            if flags & 1 and not on_host:
                raise H._lib.FtError(f'generate_batch: every x_len must be in [1, Tx = {x.shape[1]}]')
            if flags & 2:
                raise H._lib.FtError('generate_batch: token id 0 inside a sentence (t < x_len[b]); valid tokens are non-zero')
            mel, mel_post = self._ragged_finish(h, pred['mel_len'])
            out = {'mel': mel, 'mel_post': mel_post, 'mel_len': pred['mel_len'], 'dur': pred['dur'],
                   'pitch': pred['pitch'], 'energy': pred['energy']}
            if 'pitch_cond' in pred:
                out['pitch_cond'] = pred['pitch_cond']
            return out

    def _ragged_predict(self, x: torch.Tensor, xl: torch.Tensor, alpha: float, pitch_function, energy_function,
                        semb: Optional[torch.Tensor] = None):
        """the predictors, in generate()'s order; everything they hand on is zero at t >= x_len[b]
        -> dur [B,Tx] (in its returned form), mel_len, bad (the flag word), pitch / energy [B,1,Tx].
        semb (the speaker-conditioned models): pitch_cond first, the per-token argmax of its predictor's logits (-> the
        key `pitch_cond`, int64 [B,Tx]), which conditions dur and pitch; then dur, pitch, energy."""
        B, Tx = x.shape
        spk, cond, out = (), {}, {}
        if semb is not None:
            # multi_fast_pitch.py:255 divides these logits by alpha: that cannot move an argmax for alpha > 0, no launch for it
            pitch_cond = H.argmax_lens(self.pitch_cond_pred.forward_lens(x, xl, semb), xl)
            spk, cond, out = (semb,), {'x_cond': pitch_cond}, {'pitch_cond': pitch_cond}
        dur = self.dur_pred.forward_lens(x, xl, *spk, **cond, alpha=alpha).reshape(B, Tx)
        mel_len, bad = H.gen_durations(dur, xl)                   # per-item fallback, clamp; raises bit 1 of bad
        if self.checks_tokens:
            H.check_tokens_lens(x, xl, bad)                       # raises bit 2
        out.update(dur=dur, mel_len=mel_len, bad=bad)
        for key, pred, fn, kw in (('pitch', self.pitch_pred, pitch_function, cond), ('energy', self.energy_pred, energy_function, {})):
            out[key] = self._masked_user_series(key, fn, pred.forward_lens(x, xl, *spk, **kw).transpose(1, 2), xl)
        return out

    def _cond_add(self, h: torch.Tensor, pitch: torch.Tensor, energy: torch.Tensor, x_time_major: bool) -> torch.Tensor:
        """h + the model's pitch / energy projections of pitch, energy ([B,Tx] or [B,1,Tx]) -> [B,Tx,C]"""
        B = pitch.shape[0]
        return ops.CondAddFn.apply(h, pitch.reshape(B, -1), energy.reshape(B, -1), self.pitch_proj.weight,
                                   self.pitch_proj.bias, self.energy_proj.weight, self.energy_proj.bias,
                                   self.pitch_strength, self.energy_strength, x_time_major)

    def _check_ragged_batch(self, x: torch.Tensor, x_len: torch.Tensor) -> bool:
        """argument checks of generate_batch; an x_len on the host is range-checked here -> whether it was"""
        if x.dim() != 2 or x_len.dim() != 1 or x_len.numel() != x.shape[0] or x_len.dtype != torch.int64:
            raise H._lib.FtError(f'generate_batch: x must be [B,Tx] and x_len int64 [B] (got {tuple(x.shape)}, '
                                 f'{tuple(x_len.shape)} {x_len.dtype})')
        B, Tx = x.shape
        on_host = not x_len.is_cuda
        if on_host and (B == 0 or int(x_len.min()) < 1 or int(x_len.max()) > Tx):
            raise H._lib.FtError(f'generate_batch: every x_len must be in [1, Tx = {Tx}] (got {x_len.tolist()})')
        self._require_device(x)
        return on_host

    def _check_speaker_rows(self, x: torch.Tensor, speaker_emb: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the speaker rows of generate_batch -> the keyword the speaker-conditioned models' hooks get ({} for the others)"""
        S = self.speaker_emb_dims
        if not S:
            if speaker_emb is not None:
                raise H._lib.FtError(f'generate_batch: {type(self).__name__} is not speaker-conditioned, it takes no speaker_emb')
            return {}
        t = speaker_emb
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (x.shape[0], S) \
                or t.device != x.device:
            what = f'{tuple(t.shape)} {t.dtype} on {t.device}' if torch.is_tensor(t) else type(t).__name__
            raise H._lib.FtError(f'generate_batch: speaker_emb must be float32 [B = {x.shape[0]}, {S}] on {x.device}, one row '
                                 f'per item (got {what})')
        return {'semb': t.contiguous()}

    def _masked_user_series(self, key: str, fn: Callable[[torch.Tensor], torch.Tensor], v: torch.Tensor,
                            lens: torch.Tensor) -> torch.Tensor:
        """pitch_function / energy_function of generate_batch on v [B,1,Tx]: shape-checked, masked again -> [B,1,Tx]"""
        B, _, Tx = v.shape
        v = fn(v)
        if tuple(v.shape) != (B, 1, Tx) or v.dtype != torch.float32 or not v.is_cuda:
            raise H._lib.FtError(f'generate_batch: {key}_function must return a float32 device tensor of shape '
                                 f'[B,1,Tx] (got {tuple(v.shape)} {v.dtype})')
        return H.mask_rows(v.reshape(B, Tx, 1).contiguous(), lens).reshape(B, 1, Tx)

    def _bad_flag_host(self) -> torch.Tensor:
        """pinned host word the device-side generate_batch flag is copied into (asynchronously; read after the trunk's sync)"""
        if getattr(self, '_bad_host', None) is None:
            self._bad_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        return self._bad_host

    # -------------------------------------------------------------------------------------------------------------
    def get_step(self) -> int:
        return self.step.data.item()

    def pad(self, x: torch.Tensor, max_len: int) -> torch.Tensor:
        """forward_tacotron.py:236-239 on a [B,C,T] tensor (kept for API parity; forward() fuses it)."""
        x = x[:, :, :max_len]
        return torch.nn.functional.pad(x, [0, max_len - x.size(2), 0, 0], 'constant', self.padding_value)

    _pad = pad      # the name in forward_tacotron.py

    @classmethod
    def from_config(cls, config: Dict[str, Any]):
        model_config = config[cls.config_key]['model']
        model_config['num_chars'] = config.get('num_chars', NUM_CHARS_DEFAULT)   # reference: len(phonemes)
        model_config['n_mels'] = config['dsp']['num_mels']
        return cls(**model_config)

    @classmethod
    def from_checkpoint(cls, path: Union[Path, str]):
        checkpoint = torch.load(path, map_location=torch.device('cpu'), weights_only=True)
        model = cls.from_config(checkpoint['config'])
        model.load_state_dict(checkpoint['model'])
        return model
