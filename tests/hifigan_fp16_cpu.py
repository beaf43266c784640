"""HiFiGAN.matmul_dtype = 'fp16' restated on the CPU ("fp16 mode"): the oracle of
tests/test_hifigan_fp16_cpu.py and tests/test_gpu_hifigan_fp16.py.

`emulate` runs the float64 stock tree of tests/hifigan_cpu.py with the mode's operand rounding at the RESIDUAL
convolutions only -- a = fp16_rne(clamp(lrelu_0.1(x), +-65504)), w_h = fp16_rne(the weight folded in fp32) -- and float64
everywhere else (products, sums, the residual, conv_pre, the transposed convolutions, conv_post).  With rounding off it is
the float64 definition.

`resconv_h16_stage` is the float64 value of ONE kernel launch from the kernel's own fp32 input, with the a-priori bound
(K + 4) 2^-24 S + D: K the padded contraction length k cpad, S = sum |a| |w_h| (+ |bias|, the residual and the running sum
inside it, one more rounding each for the two accumulating forms), D = 2^-14 times the other operand's magnitude summed
over the terms in which a or w_h is an fp16 subnormal (what a flush of subnormal inputs could lose; zero if the hardware
keeps them)."""
import torch
import torch.nn.functional as F

import hifigan_cpu as R

FP16_MAX = 65504.0
TINY = 2.0 ** -14            # the smallest normal fp16


def operand(x):
    """x (any float dtype) -> the fp16 A operand of the mode, as float64"""
    return F.leaky_relu(x, 0.1).clamp(-FP16_MAX, FP16_MAX).to(torch.float16).double()


def weight_h(conv):
    """the weight-normed module's weight folded in fp32 and rounded to fp16 (as float64), and its bias in float64"""
    v, g = conv.weight_v.detach().float(), conv.weight_g.detach().float()
    w = v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape))
    return w.to(torch.float16).double(), conv.bias.detach().double()


def _res_conv(conv, x, rounding):
    d = conv.dilation[0]
    k = conv.kernel_size[0]
    if rounding:
        w, b = weight_h(conv)
        a = operand(x)
    else:
        w, b = R.folded(conv)
        a = F.leaky_relu(x, 0.1)
    return F.conv1d(a, w, b, dilation=d, padding=d * (k - 1) // 2)


def emulate(ref64, mel, rounding=True):
    """ref64: the float64 RefGenerator; mel [n_mels, T] -> wav [hop T] in float64"""
    x = ref64.conv_pre(mel.double().unsqueeze(0))
    nk = ref64.num_kernels
    for i in range(ref64.num_upsamples):
        x = ref64.ups[i](F.leaky_relu(x, 0.1))
        total = None
        for j in range(nk):
            blk = ref64.resblocks[i * nk + j]
            y = x
            if hasattr(blk, 'convs1'):
                for c1, c2 in zip(blk.convs1, blk.convs2):
                    y = _res_conv(c2, _res_conv(c1, y, rounding), rounding) + y
            else:
                for c in blk.convs:
                    y = _res_conv(c, y, rounding) + y
            total = y if total is None else total + y
        x = total / nk
    return torch.tanh(ref64.conv_post(F.leaky_relu(x)))[0, 0]


def resconv_h16_stage(x, d, w_h, b, res=None, prev=None, nk=1, divide=False):
    """x fp32 [C, L]; w_h float64 [C, C, k] holding fp16 values; b float64 -> (out, bound) in float64"""
    C, k = x.shape[0], w_h.shape[2]
    cpad = -(-C // 16) * 16
    a = operand(x).unsqueeze(0)
    pad = d * (k - 1) // 2
    conv = lambda u, v, bias=None: F.conv1d(u, v, bias, dilation=d, padding=pad)[0]      # noqa: E731
    out = conv(a, w_h, b)
    mag = conv(a.abs(), w_h.abs(), b.abs())
    sub_a = ((a != 0) & (a.abs() < TINY)).double()
    sub_w = ((w_h != 0) & (w_h.abs() < TINY)).double()
    flush = TINY * (conv(sub_a, w_h.abs()) + conv(a.abs(), sub_w))
    if res is not None:
        out, mag = out + res.double(), mag + res.double().abs()
    bound = (k * cpad + 4) * R.U * mag + flush
    if prev is not None:
        out, mag = out + prev.double(), mag + prev.double().abs()
        bound = bound + R.U * mag
    if divide:
        out, mag, bound = out / nk, mag / nk, bound / nk
        bound = bound + R.U * mag
    return out, bound


def unpack_h16(pack, cout, cin):
    """the fp16 pack [k, cpad / 8, CP, 8] as a numpy array -> (w [cout, cin, k], everything outside it) in numpy"""
    import numpy as np
    k, c8, CP, e = pack.shape
    full = np.ascontiguousarray(pack.transpose(0, 1, 3, 2)).reshape(k, c8 * e, CP)       # [tap, c, co]
    w = full[:, :cin, :cout].transpose(2, 1, 0)
    rest = full.copy()
    rest[:, :cin, :cout] = 0
    return w, rest
