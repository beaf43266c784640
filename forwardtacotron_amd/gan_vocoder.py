"""What the GAN vocoders (melgan.MelGAN, hifigan.HiFiGAN) share: weight-norm folding and the packed tap-major panels, the
pack cache, the checks of a mel batch, checkpoint loading, and the three entry points `inference_batch`, `inference` and
the guards of `forward`.  A generator supplies its class attributes below, its constructor and `_generate`.

Nothing here allocates a device buffer: every buffer of a call is allocated in `_generate`, through the `_empty` /
`_alloc` pair of the generator's own module (the hook the poison tests replace).
"""
import os
import warnings
from typing import Any, Callable, Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import ragged


def _wn(m: nn.Module) -> nn.Module:
    with warnings.catch_warnings():           # (the parametrization form would rename weight_g / weight_v)
        warnings.simplefilter('ignore')
        return nn.utils.weight_norm(m)


# ---- pure tensor functions (host or device; the CPU tests hold them to stock torch in float64) -------------------
def fold_weight_norm(v: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """w = v * (g / ||v||), the norm over every dimension but the first: torch._weight_norm(v, g, 0)"""
    norm = v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape)
    return v * (g / norm)


def _pad_cols(w: torch.Tensor, CP: int) -> torch.Tensor:
    out = w.new_zeros(w.shape[:-1] + (CP,))
    out[..., :w.shape[-1]] = w
    return out.contiguous()


def padded_width(cout: int) -> int:
    return -(-cout // 32) * 32


def pack_taps(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [cout, cin, k] -> tap-major panels [k, cin, CP], zero columns behind cout"""
    return _pad_cols(w.permute(2, 1, 0), padded_width(w.shape[0]))


def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """pack_taps, with k = 1 as one panel [cin, CP]"""
    p = pack_taps(w)
    return p[0].contiguous() if w.shape[2] == 1 else p


def pack_conv_transpose(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose1d weight [cin, cout, k] -> [k, cin, CP]"""
    return _pad_cols(w.permute(2, 0, 1), padded_width(w.shape[1]))


def pack_conv_out(w: torch.Tensor) -> torch.Tensor:
    """the output Conv1d's weight [1, cin, 7] -> [cin, 32], column = tap"""
    return _pad_cols(w[0], 32)


def pack_bias(b: torch.Tensor) -> torch.Tensor:
    return _pad_cols(b, padded_width(b.shape[0]))


def polyphase_taps(q: int, p: int, stride: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """ConvTranspose1d(k = 2 stride, stride, padding = stride / 2): output j = stride * q + p - stride / 2 (0 <= p <
    stride) is x[q] w[.., p] + x[q - 1] w[.., p + stride] -> ((input row, kernel tap), (input row, kernel tap)); rows
    outside the input are zero"""
    return (q, p), (q - 1, p + stride)


class GanVocoder(nn.Module):
    """Subclasses set NAME (for messages), CHECKPOINT_KEY, TAIL (frames `inference_batch` appends and cuts again) and
    MIN_FORWARD (frames `forward` needs, with the reason); give `n_mels`, `hop_length` and `_conv_out` (the output
    convolution) as attributes or properties; and implement _generate(mel, ml, tail, err, keep)."""
    NAME = ''
    CHECKPOINT_KEY = ''
    TAIL = 0
    MIN_FORWARD: Optional[Tuple[int, str]] = None

    def __init__(self) -> None:
        super().__init__()
        self._packs: Dict[Any, Any] = {}
        self._len_flag = ragged.LenFlag()                  # the pinned word a device-side mel_len check reports through

    # ------------------------------------------------------------------------------------------------
    @classmethod
    def _load_checkpoint(cls, path: Union[str, os.PathLike], make: Callable[[], 'GanVocoder'], fit_error: bool):
        """a file that holds the generator's state_dict directly or under CHECKPOINT_KEY, into make(): every entry must
        be there and none may be unknown.  fit_error: shapes of another configuration are an FtError too."""
        ck = torch.load(path, map_location='cpu')
        key = cls.CHECKPOINT_KEY
        state = ck[key] if isinstance(ck, dict) and key in ck else ck
        voc = make()
        try:
            missing, unexpected = voc.load_state_dict(state, strict=False)
        except RuntimeError as e:
            if not fit_error:
                raise
            raise _lib.FtError(f'{cls.NAME}.from_checkpoint: {path} does not fit the configuration: {str(e)[:400]}') from None
        if missing or unexpected:
            raise _lib.FtError(f'{cls.NAME}.from_checkpoint: {path} lacks {sorted(missing)} and has unknown {sorted(unexpected)}')
        return voc

    # ------------------------------------------------------------------------------------------------
    def _pack(self, key, srcs: Sequence[torch.Tensor], make):
        """weight-derived operands, rebuilt when a source tensor changes (in-place updates bump _version)"""
        tag = tuple((s.data_ptr(), s._version, s.device) for s in srcs)
        hit = self._packs.get(key)
        if hit is None or hit[0] != tag:
            hit = (tag, make())
            self._packs[key] = hit
        return hit[1]

    def _panel(self, conv: nn.Module, pack=pack_taps) -> Tuple[torch.Tensor, torch.Tensor]:
        """(packed folded weight, padded bias) of one weight-normed convolution"""
        v, g, b = conv.weight_v, conv.weight_g, conv.bias

        def make():
            with torch.no_grad():
                return pack(fold_weight_norm(v, g)), pack_bias(b)
        return self._pack(id(conv), (v, g, b), make)

    def _out_panel(self) -> Tuple[torch.Tensor, float]:
        conv = self._conv_out
        v, g, b = conv.weight_v, conv.weight_g, conv.bias

        def make():
            with torch.no_grad():                          # (the one read-back: once per parameter version)
                return pack_conv_out(fold_weight_norm(v, g)), float(b.detach().cpu()[0])
        return self._pack('out', (v, g, b), make)

    def _device(self) -> torch.device:
        dev = self._conv_out.bias.device
        if dev.type != 'cuda' or any(p.device != dev or p.dtype != torch.float32 for p in self.parameters()):
            raise _lib.FtError(f'{self.NAME} runs on an MI355X (HIP) device only, in float32; there is no CPU fallback: '
                               "move it with .to('cuda')")
        return dev

    def _check_mel(self, what: str, mel) -> None:
        if not isinstance(mel, torch.Tensor) or mel.dim() != 3:
            raise _lib.FtError(f'{what}: mel must be a [B, n_mels, Tmax] tensor')
        if mel.dtype != torch.float32:
            raise _lib.FtError(f'{what}: mel must be float32, got {mel.dtype}')
        if mel.shape[1] != self.n_mels:
            raise _lib.FtError(f'{what}: expected {self.n_mels} mel channels, got {mel.shape[1]}')
        if mel.shape[0] < 1 or mel.shape[2] < 1:
            raise _lib.FtError(f'{what}: an empty batch')
        if torch.is_grad_enabled() and (mel.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise _lib.FtError(f'{self.NAME}.{what} is an inference path (no autograd graph): call it under '
                               'torch.no_grad(), or with an input and parameters that do not require grad')

    def _generate(self, mel: torch.Tensor, ml: Optional[torch.Tensor], tail: int, err: Optional[torch.Tensor],
                  keep: bool) -> Dict[str, Any]:
        """the generator over a batch -> {'wav', 'wav_int16'} and, with keep, 'stages'"""
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------------
    def inference_batch(self, mel: torch.Tensor, mel_len: torch.Tensor, keep_stages: bool = False) -> Dict[str, Any]:
        """The published inference for a RAGGED batch (generate_batch's 'mel_post' and 'mel_len'): item b is what the
        published generator gives mel[b:b+1, :, :mel_len[b]] alone (the class docstring says what that is), times 32768,
        clamped to [-32768, 32767], truncated to int16.

        mel: float32 [B, n_mels, Tmax] on the device; what lies at t >= mel_len[b] (padding, NaN, Inf) is never loaded.
        mel_len: int64 [B], on the host or the device, 1 <= mel_len[b] <= Tmax.
        -> {'wav': float32 [B, hop * Tmax], the tanh output before quantisation, exactly 0 at j >= wav_len[b];
            'wav_len': int64 [B] = hop * mel_len on the device; 'wav_int16': int16 [B, hop * Tmax]}, hop = hop_length.
        keep_stages adds 'stages', kernel outputs in order (for the tests; which ones: the generator's _generate).

        An item's samples are bit-identical alone (Tmax its own length) and in any batch at any position.  Lengths follow
        ragged.py: a host-side mel_len is checked up front and nothing synchronises; a device-side one is clamped inside
        the kernels and its FtError is raised at the end of the call, after one synchronisation, through ONE pinned host
        word kept on this object."""
        what = 'inference_batch'
        self._check_mel(what, mel)
        B, _, Tmax = mel.shape
        if not isinstance(mel_len, torch.Tensor) or mel_len.dim() != 1 or mel_len.numel() != B or \
                mel_len.dtype != torch.int64:
            raise _lib.FtError(f'{what}: mel_len must be an int64 tensor [B = {B}]')
        if not mel_len.is_cuda and (int(mel_len.min()) < 1 or int(mel_len.max()) > Tmax):
            raise _lib.FtError(f"{ragged.range_message(what, 'mel_len', 1, Tmax, 'Tmax')} (got {mel_len.tolist()})")
        dev = self._device()
        if not mel.is_cuda:
            raise _lib.FtError(f'{what}: mel must be on the HIP device')
        mel = mel.contiguous()
        ml, err = ragged.device_lens(mel_len, B, 1, Tmax, what, 'mel_len', 'Tmax', dev)
        out = self._generate(mel, ml, self.TAIL, err, keep_stages)
        out['wav_len'] = ml * self.hop_length
        self._len_flag.check(err, ragged.range_message(what, 'mel_len', 1, Tmax, 'Tmax'))
        return out

    def inference(self, mel: torch.Tensor) -> np.ndarray:
        """the published inference of one mel, [n_mels, T] or [1, n_mels, T] on the device -> int16 numpy [hop * T]"""
        if isinstance(mel, torch.Tensor) and mel.dim() == 2:
            mel = mel.unsqueeze(0)
        if not isinstance(mel, torch.Tensor) or mel.dim() != 3 or mel.shape[0] != 1:
            raise _lib.FtError('inference: one mel, [n_mels, T] or [1, n_mels, T] (a batch goes through inference_batch)')
        out = self.inference_batch(mel, torch.tensor([mel.shape[2]], dtype=torch.int64))
        return out['wav_int16'][0].cpu().numpy()

    def forward(self, mel: torch.Tensor) -> torch.Tensor:
        """the generator without a tail: float32 [B, n_mels, T] on the device -> [B, 1, hop * T].  Inference only; every
        item has T frames."""
        self._check_mel('forward', mel)
        self._device()
        if not mel.is_cuda:
            raise _lib.FtError('forward: mel must be on the HIP device')
        if self.MIN_FORWARD is not None and mel.shape[2] < self.MIN_FORWARD[0]:
            raise _lib.FtError(f'forward: at least {self.MIN_FORWARD[0]} frames ({self.MIN_FORWARD[1]})')
        return self._generate(mel.contiguous(), None, 0, None, False)['wav'].unsqueeze(1)
