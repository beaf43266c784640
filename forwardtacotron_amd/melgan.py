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
(w = g v / ||v||) is folded into packed tap-major panels once per parameter version (gan_vocoder.py, which also holds
what this generator shares with hifigan.HiFiGAN; the fold and pack functions are re-exported here).

A RAGGED batch goes through `inference_batch(mel, mel_len)`; how mel_len is taken from the host or the device is the
contract of ragged.py.  An item's samples are bit-identical alone and inside any batch, at any position, and nothing at
t >= mel_len[b] is ever loaded.
"""
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import hip as H
from .gan_vocoder import GanVocoder, _wn, pack_conv, pack_conv_transpose
from .gan_vocoder import fold_weight_norm, pack_bias, pack_conv_out, padded_width, polyphase_taps  # noqa: F401 (re-exported)

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


def wav_length(mel_len, upsampling: int = 256):
    """samples `inference` returns for mel_len frames: upsampling * (mel_len + 10) generated, upsampling * 10 cut"""
    return upsampling * (mel_len + TAIL_FRAMES) - upsampling * TAIL_FRAMES


class MelGAN(GanVocoder):
    """`inference_batch` is the hub model's `inference` per item: ten frames of -11.5129 appended, the generator over
    (mel + 5) / 5, the last 2,560 samples cut; `forward` is the generator without that tail.  'stages' holds every
    kernel's output in order.  The shared entry points are gan_vocoder.GanVocoder's."""
    NAME = 'MelGAN'
    CHECKPOINT_KEY = 'model_g'              # the published checkpoint's key
    TAIL = TAIL_FRAMES
    MIN_FORWARD = (4, 'ReflectionPad1d(3)')

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

    n_mels = property(lambda self: self.mel_channel)
    _conv_out = property(lambda self: self.generator[16])

    @classmethod
    def from_checkpoint(cls, path: Union[str, os.PathLike], **kw) -> 'MelGAN':
        """a file that holds the generator's state_dict directly or under 'model_g' (the published checkpoint's key).
        Every one of the 126 entries must be there.  **Tested on a synthetic file of that layout only.**"""
        return cls._load_checkpoint(path, lambda: cls(**kw), fit_error=False)

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


__all__ = ['MelGAN', 'ResStack', 'fold_weight_norm', 'pack_bias', 'pack_conv', 'pack_conv_out', 'pack_conv_transpose',
           'padded_width', 'polyphase_taps', 'wav_length', 'PAD_VALUE', 'TAIL_FRAMES']
