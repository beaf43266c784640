"""HiFi-GAN vocoder on the MI355X: the `Generator` of jik876/hifi-gan, the third vocoder the reference writes mels for
(gen_forward.py:31-37,109-116) and the one behind its headline samples, taken by its published definition (DESIGN.md
section 7, "HiFi-GAN vocoder").

    voc = HiFiGAN.from_checkpoint(path, config='config.json').cuda().eval()
    with torch.no_grad():
        out = voc.inference_batch(gen['mel_post'], gen['mel_len'])        # generate_batch's output, on the device
    out['wav_int16'][b, :out['wav_len'][b]]                                # what the published inference script writes

**UNVERIFIED against the published model / checkpoint.**  Neither the published package nor a checkpoint of it is
available where this was written: parity with the published generator and the loading of a real checkpoint are
untested.  What is pinned is the written definition, restated from stock torch modules in tests/hifigan_cpu.py.

The module's parameter tree and state_dict keys are the published generator's (`conv_pre.weight_g`,
`ups.0.weight_v`, `resblocks.4.convs1.2.bias`, `conv_post.bias`, ...: 234 entries for V1 and V2, 69 for V3); it is built
from the stock torch modules in the published order, so keys, shapes and initialisation under a seed are the stock
tree's (torch's default initialisation: the published constructor's init_weights pass is not restated).  Those modules
are parameter containers: their forward raises.  Every computation is a kernel of csrc/ft_hifigan.hip: the input
convolution, LeakyReLU + transposed convolution in polyphase form, the residual convolution (or ResBlock1's fused pair
where the plan picks it) with the average over a stage's parallel blocks folded into each block's last launch, and the
output stage (tanh, zero padding behind wav_len and int16 in one pass).  Weight norm is folded into packed tap-major
panels once per parameter version; the fold and pack functions, the pack cache and the entry points are those of
gan_vocoder.py, shared with melgan.MelGAN.

`voc.matmul_dtype = 'fp16'` (default 'fp32') runs every residual convolution with fp16 matrix operands on
csrc/ft_hifigan_h16.hip: a = fp16(clamp(lrelu(x))) and fp16 weights, fp32 accumulation, fp32 residual and fp32 activations
in memory; ResBlock1's pairs are then two launches each.  conv_pre, the transposed convolutions and conv_post stay fp32.
The arithmetic, its error and its measured time: DESIGN.md section 7, "fp16 mode".

A RAGGED batch goes through `inference_batch(mel, mel_len)`; how mel_len is taken from the host or the device is the
contract of ragged.py.  An item's samples are bit-identical alone and inside any batch, at any position, and nothing at
t >= mel_len[b] is ever loaded.
"""
import json
import os
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import hip as H
from .gan_vocoder import GanVocoder, _wn, fold_weight_norm, pack_bias, pack_conv_transpose

MAX_WAV_VALUE = 32768.0
LRELU_SLOPE = 0.1
# the launch plan's limits (csrc/ft_voc_plan.h, read from the library)
MAX_KERNEL = H.HIFIGAN_MAX_KERNEL   # taps of a residual convolution: odd, at most 11
MAX_HALO = H.HIFIGAN_MAX_HALO       # rows a residual convolution reaches to either side: dilation * (k - 1) / 2 <= 40
CONFIG_KEYS = ('resblock', 'upsample_rates', 'upsample_kernel_sizes', 'upsample_initial_channel', 'resblock_kernel_sizes',
               'resblock_dilation_sizes', 'num_mels')
V1 = dict(resblock='1', upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), upsample_initial_channel=512,
          resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)), num_mels=80)
V2 = dict(V1, upsample_initial_channel=128)
V3 = dict(resblock='2', upsample_rates=(8, 8, 4), upsample_kernel_sizes=(16, 16, 8), upsample_initial_channel=256,
          resblock_kernel_sizes=(3, 5, 7), resblock_dilation_sizes=((1, 2), (2, 6), (3, 12)), num_mels=80)


def _empty(*shape, dtype=torch.float32, device=None) -> torch.Tensor:
    """every device buffer of the vocoder is allocated here (tests replace it with a poison-filling allocator)"""
    return torch.empty(*shape, dtype=dtype, device=device)


def _alloc(*shape, **kw) -> torch.Tensor:
    return _empty(*shape, **kw)               # looked up at call time, so a replaced _empty takes effect


def _container(self, *a, **kw):
    raise _lib.FtError('HiFiGAN: the stock modules are parameter containers; use HiFiGAN.forward / inference_batch')


def _conv(ch: int, k: int, d: int) -> nn.Module:
    return _wn(nn.Conv1d(ch, ch, k, 1, dilation=d, padding=d * (k - 1) // 2))


class ResBlock1(nn.Module):
    """for m: x = x + convs2[m](lrelu(convs1[m](lrelu(x)))), convs1[m] at dilation d[m], convs2[m] at dilation 1"""

    def __init__(self, channels: int, kernel_size: int, dilation: Sequence[int]) -> None:
        super().__init__()
        self.convs1 = nn.ModuleList([_conv(channels, kernel_size, d) for d in dilation])
        self.convs2 = nn.ModuleList([_conv(channels, kernel_size, 1) for _ in dilation])

    forward = _container


class ResBlock2(nn.Module):
    """for m: x = x + convs[m](lrelu(x)), convs[m] at dilation d[m]"""

    def __init__(self, channels: int, kernel_size: int, dilation: Sequence[int]) -> None:
        super().__init__()
        self.convs = nn.ModuleList([_conv(channels, kernel_size, d) for d in dilation])

    forward = _container


pair_is_fused = H.hifigan_pair_is_fused
MATMUL_DTYPES = ('fp32', 'fp16')
FP16_MAX = 65504.0


def pack_taps_h16(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [cout, cin, k] (fp32, folded) -> the fp16 pack of ft_hifigan_resconv_h16, [k, cpad / 8, CP, 8]:
    element [tap, c // 8, co, c % 8] = fp16_rne(w[co, c, tap]), cpad = cin rounded up to 16 and CP = cout rounded up to
    32, exact zeros behind cin and cout.  A lane's B fragment (8 consecutive input channels of one output channel) is
    16 contiguous bytes, and the 32 output channels of a tile follow each other."""
    cout, cin, k = w.shape
    cpad, CP = -(-cin // 16) * 16, -(-cout // 32) * 32
    full = torch.zeros(k, cpad, CP, dtype=torch.float16, device=w.device)
    full[:, :cin, :cout] = w.permute(2, 1, 0).to(torch.float16)
    return full.reshape(k, cpad // 8, 8, CP).permute(0, 1, 3, 2).contiguous()


class HiFiGAN(GanVocoder):
    """`inference_batch` is the published inference per item: `generator(mel[b:b+1, :, :mel_len[b]]).squeeze() * 32768`
    of the mel as it is (no normalisation), clamped to [-32768, 32767] (the published script does not clamp: DESIGN.md,
    "Deviations"); `forward` is generator(mel).  'stages' holds the outputs of conv_pre and, per upsampling stage, of the
    transposed convolution and of the averaged residual blocks.  The shared entry points are gan_vocoder.GanVocoder's."""
    NAME = 'HiFiGAN'
    CHECKPOINT_KEY = 'generator'            # the published checkpoint's key

    def __init__(self, resblock: Union[str, int] = '1', upsample_rates: Sequence[int] = (8, 8, 2, 2),
                 upsample_kernel_sizes: Sequence[int] = (16, 16, 4, 4), upsample_initial_channel: int = 512,
                 resblock_kernel_sizes: Sequence[int] = (3, 7, 11),
                 resblock_dilation_sizes: Sequence[Sequence[int]] = ((1, 3, 5), (1, 3, 5), (1, 3, 5)),
                 num_mels: int = 80) -> None:
        super().__init__()
        resblock = str(resblock)
        rates = tuple(int(u) for u in upsample_rates)
        kernels = tuple(int(k) for k in upsample_kernel_sizes)
        rk = tuple(int(k) for k in resblock_kernel_sizes)
        rd = tuple(tuple(int(d) for d in ds) for ds in resblock_dilation_sizes)
        C0, num_mels = int(upsample_initial_channel), int(num_mels)
        if resblock not in ('1', '2'):
            raise _lib.FtError(f"HiFiGAN: resblock must be '1' or '2', got {resblock!r}")
        if not rates or len(rates) != len(kernels):
            raise _lib.FtError('HiFiGAN: one upsample kernel size per upsample rate, at least one')
        if any(k != 2 * u or u < 2 or u % 2 for u, k in zip(rates, kernels)):
            raise _lib.FtError(f'HiFiGAN: every transposed convolution must have kernel = 2 rate with an even rate (the '
                               f'two-tap polyphase form, padding = rate / 2), got rates {rates}, kernels {kernels}')
        if not rk or len(rk) != len(rd) or any(len(ds) < 1 for ds in rd):
            raise _lib.FtError('HiFiGAN: one non-empty dilation list per resblock kernel size, at least one')
        if any(k < 1 or k % 2 == 0 or k > MAX_KERNEL for k in rk):
            raise _lib.FtError(f'HiFiGAN: resblock kernel sizes must be odd and at most {MAX_KERNEL}, got {rk}')
        for k, ds in zip(rk, rd):
            if any(d < 1 or d * (k - 1) // 2 > MAX_HALO for d in ds):
                raise _lib.FtError(f'HiFiGAN: a dilation of {ds} with {k} taps reaches {max(ds) * (k - 1) // 2} rows to '
                                   f'either side; the plan supports a halo of at most {MAX_HALO} rows (dilation >= 1)')
        widths = tuple(C0 >> (i + 1) for i in range(len(rates)))
        if num_mels % 8 or not 8 <= num_mels <= 128 or C0 % 8 or not 8 <= C0 <= 512 or \
                any(c % 8 or c < 8 or (c << (i + 1)) != C0 for i, c in enumerate(widths)) or max(widths) > 256 or \
                widths[-1] > 32:
            raise _lib.FtError(f'HiFiGAN: widths must be multiples of 8 with num_mels <= 128, upsample_initial_channel <= '
                               f'512 at conv_pre, the residual stages <= 256 and the last <= 32 (got {num_mels}, {C0} -> '
                               f'{widths})')
        self.resblock, self.upsample_rates, self.upsample_kernel_sizes = resblock, rates, kernels
        self.upsample_initial_channel, self.resblock_kernel_sizes, self.resblock_dilation_sizes = C0, rk, rd
        self.num_mels, self.widths = num_mels, widths
        self.hop_length = int(np.prod(rates))
        block = ResBlock1 if resblock == '1' else ResBlock2
        self.conv_pre = _wn(nn.Conv1d(num_mels, C0, 7, 1, padding=3))
        self.ups = nn.ModuleList([_wn(nn.ConvTranspose1d(C0 >> i, C0 >> (i + 1), k, u, padding=(k - u) // 2))
                                  for i, (u, k) in enumerate(zip(rates, kernels))])
        self.resblocks = nn.ModuleList([block(c, k, ds) for c in widths for k, ds in zip(rk, rd)])
        self.conv_post = _wn(nn.Conv1d(widths[-1], 1, 7, 1, padding=3))

    n_mels = property(lambda self: self.num_mels)
    _conv_out = property(lambda self: self.conv_post)

    @property
    def matmul_dtype(self) -> str:
        """'fp32' (default): every product on the exact-fp32 MFMA.  'fp16': the residual convolutions take fp16 operands
        ("fp16 mode"); conv_pre, the transposed convolutions and conv_post stay fp32.  Not part of
        the state_dict."""
        return getattr(self, '_matmul_dtype', 'fp32')

    @matmul_dtype.setter
    def matmul_dtype(self, value: str) -> None:
        if value not in MATMUL_DTYPES:
            raise _lib.FtError(f"HiFiGAN.matmul_dtype must be one of {MATMUL_DTYPES}, got {value!r}")
        object.__setattr__(self, '_matmul_dtype', value)

    def _panel_h16(self, conv: nn.Module):
        """(fp16 pack of the folded weight, padded fp32 bias) of one residual convolution: the fold stays in fp32, the
        pack has its own cache key, and a folded weight beyond fp16's range is refused here (one read-back per
        parameter version)"""
        v, g, b = conv.weight_v, conv.weight_g, conv.bias

        def make():
            with torch.no_grad():
                w = fold_weight_norm(v, g)
                wh = w.to(torch.float16)
                if not bool(torch.isfinite(wh).all()):
                    raise _lib.FtError(f"HiFiGAN: matmul_dtype = 'fp16' needs folded weights that are finite in fp16 (|w| <= "
                                       f'{FP16_MAX:.0f}); largest |w| here: {float(w.abs().max()):.4g}')
                return pack_taps_h16(w), pack_bias(b)
        return self._pack(('h16', id(conv)), (v, g, b), make)

    # ------------------------------------------------------------------------------------------------
    @classmethod
    def from_config(cls, config: Union[Dict[str, Any], str, os.PathLike]) -> 'HiFiGAN':
        """the published config.json, as a dict or a path: the generator's keys are taken, the training keys ignored"""
        if not isinstance(config, dict):
            with open(config) as f:
                config = json.load(f)
        return cls(**{k: config[k] for k in CONFIG_KEYS if k in config})

    @classmethod
    def v1(cls) -> 'HiFiGAN':
        return cls(**V1)

    @classmethod
    def v2(cls) -> 'HiFiGAN':
        return cls(**V2)

    @classmethod
    def v3(cls) -> 'HiFiGAN':
        return cls(**V3)

    @classmethod
    def from_checkpoint(cls, path: Union[str, os.PathLike], config: Union[None, Dict[str, Any], str, os.PathLike] = None
                        ) -> 'HiFiGAN':
        """a file that holds the generator's state_dict directly or under 'generator' (the published checkpoint's key);
        config: the published config.json as a dict or a path (default: V1).  Every entry must be there and none may be
        unknown.  **Tested on a synthetic file of that layout only.**"""
        return cls._load_checkpoint(path, lambda: cls.v1() if config is None else cls.from_config(config), fit_error=True)

    def _stage(self, i: int, x: torch.Tensor, ml: Optional[torch.Tensor], B: int, Tmax: int, scale: int) -> torch.Tensor:
        """(sum over j of resblocks[i nk + j](x), j ascending) / nk.  Each block's last launch writes the stage's buffer:
        block 0 stores, the later ones add, the last one divides; the launches are ordered on the current stream."""
        nk = len(self.resblock_kernel_sizes)
        h16 = self.matmul_dtype == 'fp16'
        total = _alloc(*x.shape, dtype=torch.float32, device=x.device)
        tmp: List[Optional[torch.Tensor]] = [None, None, None]          # two buffers in turn for the chain, one for mid

        def buf(n: int) -> torch.Tensor:
            if tmp[n] is None:
                tmp[n] = _alloc(*x.shape, dtype=torch.float32, device=x.device)
            return tmp[n]
        for j, (k, ds) in enumerate(zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes)):
            blk = self.resblocks[i * nk + j]
            y = x
            for m, d in enumerate(ds):
                last = m == len(ds) - 1
                out = total if last else buf(m % 2)
                acc = 0 if not last or j == 0 else 1
                if last and j == nk - 1 and nk > 1:
                    acc = 2
                kw = dict(acc_mode=acc, nk=nk, out=out, alloc=_alloc)
                if h16:                                       # fp16 operands: every convolution is its own launch
                    if self.resblock == '2':
                        w, b = self._panel_h16(blk.convs[m])
                        H.hifigan_resconv_h16(y, ml, B, Tmax, scale, d, w, b, res='x', **kw)
                    else:
                        w1, b1 = self._panel_h16(blk.convs1[m])
                        w2, b2 = self._panel_h16(blk.convs2[m])
                        mid = H.hifigan_resconv_h16(y, ml, B, Tmax, scale, d, w1, b1, out=buf(2), alloc=_alloc)
                        H.hifigan_resconv_h16(mid, ml, B, Tmax, scale, 1, w2, b2, res=y, **kw)
                elif self.resblock == '2':
                    w, b = self._panel(blk.convs[m])
                    H.hifigan_resconv(y, ml, B, Tmax, scale, d, w, b, res='x', **kw)
                else:
                    w1, b1 = self._panel(blk.convs1[m])
                    w2, b2 = self._panel(blk.convs2[m])
                    if pair_is_fused(x.shape[1], k, d):
                        H.hifigan_respair(y, ml, B, Tmax, scale, d, w1, b1, w2, b2, **kw)
                    else:
                        mid = H.hifigan_resconv(y, ml, B, Tmax, scale, d, w1, b1, out=buf(2), alloc=_alloc)
                        H.hifigan_resconv(mid, ml, B, Tmax, scale, 1, w2, b2, res=y, **kw)
                y = out
        return total

    def _generate(self, mel: torch.Tensor, ml: Optional[torch.Tensor], tail: int, err: Optional[torch.Tensor],
                  keep: bool) -> Dict[str, Any]:
        """the generator over a batch (tail is always 0) -> {'wav', 'wav_int16'} and, with keep, 'stages': the input
        convolution's output, then per upsampling stage the transposed convolution's and the averaged residual blocks'"""
        B, _, Tmax = mel.shape
        stages: List[torch.Tensor] = []
        w, b = self._panel(self.conv_pre)
        x = H.hifigan_conv_in(mel, ml, w, b, self.upsample_initial_channel, err, alloc=_alloc)
        stages.append(x)
        scale = 1
        for i, u in enumerate(self.upsample_rates):
            w, b = self._panel(self.ups[i], pack_conv_transpose)
            x = H.hifigan_upsample(x, ml, B, Tmax, scale, u, w, b, self.widths[i], alloc=_alloc)
            scale *= u
            stages.append(x)
            x = self._stage(i, x, ml, B, Tmax, scale)
            stages.append(x)
        wo, bo = self._out_panel()
        wav, i16 = H.hifigan_conv_out(x, ml, B, Tmax, scale, wo, bo, alloc=_alloc)
        out = {'wav': wav, 'wav_int16': i16}
        if keep:
            out['stages'] = stages
        return out


__all__ = ['HiFiGAN', 'ResBlock1', 'ResBlock2', 'pair_is_fused', 'pack_taps_h16', 'MATMUL_DTYPES', 'V1', 'V2', 'V3', 'MAX_HALO', 'MAX_KERNEL']
