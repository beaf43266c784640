"""MelGAN vocoder on the MI355X: the generator of seungwonpark/melgan, the network behind the reference's
`Synthesizer` (notebook_utils/synthesize.py:22,46-48: `torch.hub.load('seungwonpark/melgan', 'melgan')`,
`self.melgan.inference(mel_post)`), taken by its published definition ("MelGAN vocoder").

    voc = MelGAN.from_checkpoint(path).cuda().eval()
    with torch.no_grad():
        out = voc.inference_batch(gen['mel_post'], gen['mel_len'])        # generate_batch's output, on the device
    out['wav_int16'][b, :out['wav_len'][b]]                                # what the hub model's inference() returns

**UNVERIFIED against the published model.**  Neither the hub package nor its checkpoint is available where this was
written: parity with the published generator and the loading of its real checkpoint are untested.  What is pinned is the
written definition, restated from stock torch modules in tests/melgan_cpu.py.

The module's parameter tree and state_dict keys are the published generator's (`generator.1.weight_g`,
`generator.4.blocks.0.2.weight_v`, `generator.4.shortcuts.0.bias`, ...: 126 entries); it is built from the stock torch
modules in the published order, so initialisation under a seed is that of the stock tree.  Those modules are parameter
containers: their forward is never called.  Every computation is one of the four kernels of csrc/ft_melgan.hip: the
input convolution (normalisation and the ten appended frames on load), LeakyReLU + transposed convolution in polyphase
form, the fused residual block, and the output stage (tanh, tail cut, zero padding and int16 in one pass).  Weight norm
(w = g v / ||v||) is folded into packed tap-major panels once per parameter version.

A RAGGED batch goes through `inference_batch(mel, mel_len)`; how mel_len is taken from the host or the device is the
contract of ragged.py.  An item's samples are bit-identical alone and inside any batch, at any position, and nothing at
t >= mel_len[b] is ever loaded.
"""
import os
import warnings
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import hip as H
from . import ragged

PAD_VALUE = -11.5129            # ln(1e-5): the floor of the reference's mel and the value of the appended frames
TAIL_FRAMES = 10                # frames `inference` appends and whose samples it cuts again
MAX_WAV_VALUE = 32768.0
LRELU_SLOPE = 0.2
DILATIONS = (1, 3, 9)


def _empty(*shape, dtype=torch.float32, device=None) -> torch.Tensor:
    """every device buffer of the vocoder is allocated here (tests replace it with a poison-filling allocator)"""
    return torch.empty(*shape, dtype=dtype, device=device)


def _alloc(*shape, **kw) -> torch.Tensor:
    return _empty(*shape, **kw)               # looked up at call time, so a replaced _empty takes effect


def _wn(m: nn.Module) -> nn.Module:
    with warnings.catch_warnings():           # (the parametrization form would rename weight_g / weight_v)
        warnings.simplefilter('ignore')
        return nn.utils.weight_norm(m)


class ResStack(nn.Module):
    """three blocks: x = shortcuts[i](x) + blocks[i](x), blocks[i] = LeakyReLU, ReflectionPad1d(3^i), Conv1d(k = 3,
    dilation 3^i), LeakyReLU, Conv1d(k = 1) -- the published layout, blocks built before shortcuts"""

    def __init__(self, channel: int) -> None:
        super().__init__()
        self.blocks = nn.ModuleList([
            nn.Sequential(nn.LeakyReLU(LRELU_SLOPE), nn.ReflectionPad1d(d),
                          _wn(nn.Conv1d(channel, channel, kernel_size=3, dilation=d)),
                          nn.LeakyReLU(LRELU_SLOPE), _wn(nn.Conv1d(channel, channel, kernel_size=1)))
            for d in DILATIONS])
        self.shortcuts = nn.ModuleList([_wn(nn.Conv1d(channel, channel, kernel_size=1)) for _ in DILATIONS])

    def forward(self, *a, **kw):
        raise _lib.FtError('MelGAN: the stock modules are parameter containers; use MelGAN.forward / inference_batch')


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


def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [cout, cin, k] -> tap-major panels [k, cin, CP] (k = 1: [cin, CP]), zero columns behind cout"""
    p = _pad_cols(w.permute(2, 1, 0), padded_width(w.shape[0]))
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


def wav_length(mel_len, upsampling: int = 256):
    """samples `inference` returns for mel_len frames: upsampling * (mel_len + 10) generated, upsampling * 10 cut"""
    return upsampling * (mel_len + TAIL_FRAMES) - upsampling * TAIL_FRAMES


class MelGAN(nn.Module):
    def __init__(self, mel_channel: int = 80, channels: Sequence[int] = (512, 256, 128, 64, 32),
                 upsamples: Sequence[Tuple[int, int, int]] = ((16, 8, 4), (16, 8, 4), (4, 2, 1), (4, 2, 1))) -> None:
        super().__init__()
        channels = tuple(int(c) for c in channels)
        upsamples = tuple(tuple(int(v) for v in u) for u in upsamples)
        if len(channels) != 5 or len(upsamples) != 4 or any(len(u) != 3 for u in upsamples):
            raise _lib.FtError('MelGAN: five channel widths and four (kernel, stride, padding) triples')
        if any(k != 2 * s or 2 * p != s or s < 2 for k, s, p in upsamples):
            raise _lib.FtError(f'MelGAN: every transposed convolution must have kernel = 2 stride, padding = stride / 2 '
                               f'(the two-tap polyphase form), got {upsamples}')
        if mel_channel % 8 or not 8 <= mel_channel <= 128 or any(c % 8 or c < 8 for c in channels) or channels[0] > 512 \
                or max(channels[1:]) > 256 or channels[4] > 32:
            raise _lib.FtError(f'MelGAN: widths must be multiples of 8 with mel_channel <= 128, channels[0] <= 512, the '
                               f'residual stacks <= 256 and the last <= 32 (got {mel_channel}, {channels})')
        self.mel_channel, self.channels, self.upsamples = int(mel_channel), channels, upsamples
        self.hop_length = int(np.prod([s for _, s, _ in upsamples]))
        layers: List[nn.Module] = [nn.ReflectionPad1d(3), _wn(nn.Conv1d(mel_channel, channels[0], kernel_size=7, stride=1))]
        for i, (k, s, p) in enumerate(upsamples):
            layers += [nn.LeakyReLU(LRELU_SLOPE),
                       _wn(nn.ConvTranspose1d(channels[i], channels[i + 1], kernel_size=k, stride=s, padding=p)),
                       ResStack(channels[i + 1])]
        layers += [nn.LeakyReLU(LRELU_SLOPE), nn.ReflectionPad1d(3), _wn(nn.Conv1d(channels[4], 1, kernel_size=7, stride=1)),
                   nn.Tanh()]
        self.generator = nn.Sequential(*layers)
        self._packs: Dict[Any, Any] = {}
        self._len_flag = ragged.LenFlag()                  # the pinned word a device-side mel_len check reports through

    # ------------------------------------------------------------------------------------------------
    @classmethod
    def from_checkpoint(cls, path: Union[str, os.PathLike], **kw) -> 'MelGAN':
        """a file that holds the generator's state_dict directly or under 'model_g' (the published checkpoint's key).
        Every one of the 126 entries must be there.  **Tested on a synthetic file of that layout only.**"""
        ck = torch.load(path, map_location='cpu')
        state = ck['model_g'] if isinstance(ck, dict) and 'model_g' in ck else ck
        voc = cls(**kw)
        missing, unexpected = voc.load_state_dict(state, strict=False)
        if missing or unexpected:
            raise _lib.FtError(f'MelGAN.from_checkpoint: {path} lacks {sorted(missing)} and has unknown {sorted(unexpected)}')
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

    def _panel(self, conv: nn.Module, pack) -> Tuple[torch.Tensor, torch.Tensor]:
        """(packed folded weight, padded bias) of one weight-normed convolution"""
        v, g, b = conv.weight_v, conv.weight_g, conv.bias

        def make():
            with torch.no_grad():
                return pack(fold_weight_norm(v, g)), pack_bias(b)
        return self._pack(id(conv), (v, g, b), make)

    def _out_panel(self) -> Tuple[torch.Tensor, float]:
        conv = self.generator[16]
        v, g, b = conv.weight_v, conv.weight_g, conv.bias

        def make():
            with torch.no_grad():                          # (the one read-back: once per parameter version)
                return pack_conv_out(fold_weight_norm(v, g)), float(b.detach().cpu()[0])
        return self._pack('out', (v, g, b), make)

    def _device(self) -> torch.device:
        dev = self.generator[1].bias.device
        if dev.type != 'cuda' or any(p.device != dev or p.dtype != torch.float32 for p in self.parameters()):
            raise _lib.FtError('MelGAN runs on an MI355X (HIP) device only, in float32; there is no CPU fallback: move it '
                               "with .to('cuda')")
        return dev

    def _check_mel(self, what: str, mel) -> None:
        if not isinstance(mel, torch.Tensor) or mel.dim() != 3:
            raise _lib.FtError(f'{what}: mel must be a [B, n_mels, Tmax] tensor')
        if mel.dtype != torch.float32:
            raise _lib.FtError(f'{what}: mel must be float32, got {mel.dtype}')
        if mel.shape[1] != self.mel_channel:
            raise _lib.FtError(f'{what}: expected {self.mel_channel} mel channels, got {mel.shape[1]}')
        if mel.shape[0] < 1 or mel.shape[2] < 1:
            raise _lib.FtError(f'{what}: an empty batch')
        if torch.is_grad_enabled() and (mel.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise _lib.FtError(f'MelGAN.{what} is an inference path (no autograd graph): call it under torch.no_grad(), or '
                               'with an input and parameters that do not require grad')

    def _generate(self, mel: torch.Tensor, ml: Optional[torch.Tensor], tail: int, err: Optional[torch.Tensor],
                  keep: bool) -> Dict[str, Any]:
        """the generator over a batch -> {'wav', 'wav_int16'} and, with keep, 'stages': every kernel's output"""
        B, _, Tmax = mel.shape
        g = self.generator
        stages: List[torch.Tensor] = []
        w, b = self._panel(g[1], pack_conv)
        x = H.melgan_conv_in(mel, ml, tail, PAD_VALUE, w, b, self.channels[0], err, alloc=_alloc)
        scale = 1
        if keep:
            stages.append(x)
        for i, (_, s, _) in enumerate(self.upsamples):
            C = self.channels[i + 1]
            w, b = self._panel(g[3 * i + 3], pack_conv_transpose)
            x = H.melgan_upsample(x, ml, B, Tmax, tail, scale, s, w, b, C, alloc=_alloc)
            scale *= s
            if keep:
                stages.append(x)
            stack = g[3 * i + 4]
            spare = None
            for j, d in enumerate(DILATIONS):
                w1, b1 = self._panel(stack.blocks[j][2], pack_conv)
                w2, b2 = self._panel(stack.blocks[j][4], pack_conv)
                ws, bs = self._panel(stack.shortcuts[j], pack_conv)
                y = H.melgan_resblock(x, ml, B, Tmax, tail, scale, d, w1, b1, w2, b2, ws, bs,
                                      out=None if keep else spare, alloc=_alloc)
                x, spare = y, x
                if keep:
                    stages.append(x)
        wo, bo = self._out_panel()
        wav, i16 = H.melgan_conv_out(x, ml, B, Tmax, tail, scale, wo, bo, alloc=_alloc)
        out = {'wav': wav, 'wav_int16': i16}
        if keep:
            out['stages'] = stages
        return out

    # ------------------------------------------------------------------------------------------------
    def inference_batch(self, mel: torch.Tensor, mel_len: torch.Tensor, keep_stages: bool = False) -> Dict[str, Any]:
        """The hub model's `inference` for a RAGGED batch (generate_batch's 'mel_post' and 'mel_len'): item b is what
        inference gives mel[b:b+1, :, :mel_len[b]] alone -- ten frames of -11.5129 appended, the generator, the last
        2,560 samples cut, times 32768, clamped to [-32768, 32767], truncated to int16.

        mel: float32 [B, n_mels, Tmax] on the device; what lies at t >= mel_len[b] (padding, NaN, Inf) is never loaded.
        mel_len: int64 [B], on the host or the device, 1 <= mel_len[b] <= Tmax.
        -> {'wav': float32 [B, hop * Tmax], the tanh output before quantisation, exactly 0 at j >= wav_len[b];
            'wav_len': int64 [B] = hop * mel_len on the device; 'wav_int16': int16 [B, hop * Tmax]}, hop = 256.
        keep_stages adds 'stages', every kernel's output in order (for the tests).

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
        out = self._generate(mel, ml, TAIL_FRAMES, err, keep_stages)
        out['wav_len'] = ml * self.hop_length
        self._len_flag.check(err, ragged.range_message(what, 'mel_len', 1, Tmax, 'Tmax'))
        return out

    def inference(self, mel: torch.Tensor) -> np.ndarray:
        """the hub model's inference: one mel [n_mels, T] or [1, n_mels, T] on the device -> int16 numpy [hop * T]"""
        if isinstance(mel, torch.Tensor) and mel.dim() == 2:
            mel = mel.unsqueeze(0)
        if not isinstance(mel, torch.Tensor) or mel.dim() != 3 or mel.shape[0] != 1:
            raise _lib.FtError('inference: one mel, [n_mels, T] or [1, n_mels, T] (a batch goes through inference_batch)')
        out = self.inference_batch(mel, torch.tensor([mel.shape[2]], dtype=torch.int64))
        return out['wav_int16'][0].cpu().numpy()

    def forward(self, mel: torch.Tensor) -> torch.Tensor:
        """generator((mel + 5) / 5) without the ten-frame tail: float32 [B, n_mels, T] on the device -> [B, 1, hop * T].
        Inference only; every item has T frames."""
        self._check_mel('forward', mel)
        self._device()
        if not mel.is_cuda:
            raise _lib.FtError('forward: mel must be on the HIP device')
        if mel.shape[2] < 4:
            raise _lib.FtError('forward: at least 4 frames (ReflectionPad1d(3))')
        return self._generate(mel.contiguous(), None, 0, None, False)['wav'].unsqueeze(1)


__all__ = ['MelGAN', 'ResStack', 'fold_weight_norm', 'pack_bias', 'pack_conv', 'pack_conv_out', 'pack_conv_transpose',
           'padded_width', 'polyphase_taps', 'wav_length', 'PAD_VALUE', 'TAIL_FRAMES']
