"""MI355X-native FastPitch: drop-in for models/fast_pitch.py:14-235 and the transformer layers of
models/common_layers.py:127-223 (same constructor kwargs, batch-dict forward()/generate(), state_dict incl. the
`pe` buffers).  torch.nn.{MultiheadAttention,LayerNorm,Conv1d,Linear,Embedding} objects are parameter
containers only; every computation is a gfx950 kernel behind the C ABI:
  attention = in_proj GEMM -> strided-batch QK^T (f32 MFMA) -> masked softmax -> strided-batch PV -> out_proj,
  backward = the five transposed products (dV, dP, dQ, dK via batched NT/NN/TN GEMMs) + softmax gradient.
Activations are batch-major channels-last [B,T,d] (the reference's [T,B,d] is only a view convention).
"""
import copy
import functools
import math
import os
from typing import Callable, Dict, Optional

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib
from . import hip as H
from . import ops
from .base import AcousticModel, LengthRegulator, PAD_VALUE, _dropout, _seed, predictor_front, predictor_tail
from .gradsink import batched_side_launches, emit, installed
from .ops import _c

_F4 = 4


def _p(t):
    return None if t is None else t.data_ptr()


def _bgemm(kind, A_ptr, lda, sA0, sA1, B_ptr, ldb, sB0, sB1, C_ptr, ldc, sC0, sC1, M, N, K, nb0, nb1, device,
           padded: bool = False):
    """padded: the [T,T]-shaped operand is stored with its row stride rounded up to 4 (see MHAFn)"""
    if kind == 'tn':
        _lib.call('ft_bgemm_tn', A_ptr, lda, sA0, sA1, B_ptr, ldb, sB0, sB1, C_ptr, ldc, sC0, sC1, M, N, K, nb0, nb1,
                  int(padded), *H.scratch('ft_bgemm_tn_workspace', M, N, K, nb0, nb1, device=device), H._stream())
    elif kind == 'nn':
        _lib.call('ft_bgemm_nn', A_ptr, lda, sA0, sA1, B_ptr, ldb, sB0, sB1, C_ptr, ldc, sC0, sC1, M, N, K, nb0, nb1,
                  int(padded), H._stream())
    else:
        _lib.call('ft_bgemm_nt', A_ptr, lda, sA0, sA1, B_ptr, ldb, sB0, sB1, C_ptr, ldc, sC0, sC1, M, N, K, nb0, nb1,
                  H._stream())


def precision_scoped(fn):
    """runs a model method under the model's `matmul_dtype` ('fp32' default, 'bf16' = BASELINE configs[2])"""
    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        with H.gemm_precision(self.matmul_dtype):
            return fn(self, *a, **k)
    return wrapped


def _attn_unfused(qkv, key_pad, nh, scale, p_drop, seed):
    """softmax(scale Q K^T + key mask) V through three launches with the [B,nh,T,T] matrices in memory
    -> (att [B,T,d], P, dropout(P))"""
    B, T, d3 = qkv.shape
    d = d3 // 3
    hd = d // nh
    # the [T,T] score / probability matrices are kept with their row stride rounded up to 4 floats (pad columns
    # are zeros): T = 841 frames would otherwise push four of the six attention GEMMs off the 16-B-load paths
    Tp = (T + 3) // 4 * 4
    P = torch.empty(B, nh, T, Tp, device=qkv.device, dtype=qkv.dtype)
    q0 = qkv.data_ptr()
    _bgemm('nt', q0, 3 * d, T * 3 * d, hd, q0 + d * _F4, 3 * d, T * 3 * d, hd, P.data_ptr(), Tp, nh * T * Tp, T * Tp,
           T, T, hd, B, nh, qkv.device)
    # softmax and nn.MultiheadAttention's attention dropout in one pass; both P and dropout(P) are kept for backward
    Pd = torch.empty_like(P) if p_drop > 0 else P
    _lib.call('ft_softmax_fwd', P.data_ptr(), _p(key_pad), B, nh, T, T, Tp, scale,
              Pd.data_ptr() if p_drop > 0 else None, float(p_drop), int(seed), H._stream())
    att = torch.empty(B, T, d, device=qkv.device, dtype=qkv.dtype)
    _bgemm('nn', Pd.data_ptr(), Tp, nh * T * Tp, T * Tp, q0 + 2 * d * _F4, 3 * d, T * 3 * d, hd, att.data_ptr(), d,
           T * d, hd, T, hd, T, B, nh, qkv.device, padded=True)
    return att, P, Pd


# ft_attn_fwd_lens at the multispeaker models' head widths (192 = the unconditioned predictors' 384 on 2 heads, 256 = the
# trunk's 512 on 2 heads): whether it is the default route of a ragged batch, per matmul mode -- the outcome of the A/B in
# profiles/multi_generate_batch.txt (tools/bench_multi_generate_batch.py).  FT_ATTN_LENS=1 / 0 forces it on / off.
WIDE_LENS_DEFAULT = {'fp32': True, 'bf16': True}


def attn_route(hd: int, ragged: bool = False) -> str:
    """Which attention serves head width hd under the current matmul mode (the switches are read per call):
    'lens'    ragged batches only: ft_attn_fwd_lens reads the lengths on the device, head widths 64 / 128 in both modes
              and 192 / 256 (its wide-head layout) where WIDE_LENS_DEFAULT says so; FT_ATTN_LENS=0 forces the masked
              routes below (A/B aid), FT_ATTN_LENS=1 forces the kernel at every width it has
    'fused'   bf16 mode, head widths 64 / 128: ONE flash-style kernel between the two projections -- no [B,h,T,T] tensor
              in memory, the backward recomputes the probabilities (csrc/ft_attn.hip); FT_ATTN_FUSED=0 turns it off
    'unfused' everything else: _attn_unfused
    Head width 196 (the multispeaker models' CONDITIONED predictors, 392 on 2 heads) has no fused kernel: it only occurs
    on the token side (Tx <= ~128 keys), and stays on the masked 'unfused' route of mha_fwd_lens."""
    if ragged and hd in (64, 128, 192, 256):
        switch = os.environ.get('FT_ATTN_LENS')
        if switch == '1' or (switch is None and (hd <= 128 or WIDE_LENS_DEFAULT[H.gemm_precision_mode()])):
            return 'lens'
    if hd in (64, 128) and H.gemm_precision_mode() == 'bf16' and os.environ.get('FT_ATTN_FUSED', '1') == '1':
        return 'fused'
    return 'unfused'


def mha_fwd(x, key_pad, in_w, in_b, out_w, out_b, nheads, p_drop, seed):
    """nn.MultiheadAttention(d, nheads, dropout)(x, x, x, key_padding_mask=key_pad)[0]  (common_layers.py:172-174) on
    batch-major x [B,T,d]; key_pad uint8 [B,T] (1 = padded key) or None.  -> (out, tape for mha_bwd)"""
    B, T, d = x.shape
    nh = int(nheads)
    hd = d // nh
    scale = 1.0 / math.sqrt(hd)
    qkv = H.linear_fwd(x, in_w, in_b)                                   # [B,T,3d]
    tape = dict(x=x, qkv=qkv, key_pad=key_pad, nh=nh, hd=hd, scale=scale, p=float(p_drop), seed=int(seed))
    if attn_route(hd) == 'fused':
        att, lse2 = H.attn_fwd(qkv, key_pad, nh, scale, p_drop, seed)
        tape.update(fused=True, att=att, lse2=lse2)
        return H.linear_fwd(att, out_w, out_b), tape
    att, P, Pd = _attn_unfused(qkv, key_pad, nh, scale, p_drop, seed)
    tape.update(fused=False, att=att, P=P, Pd=Pd)
    return H.linear_fwd(att, out_w, out_b), tape


def mha_fwd_lens(x, lens, in_w, in_b, out_w, out_b, nheads):
    """Inference self-attention of a ragged batch (torch.no_grad only, no tape): x [B,T,d], lens int64 [B] on the device.
    Rows t < lens[b] attend to keys < lens[b] only; the attention output is exactly 0 at t >= lens[b] (the result holds
    the out-projection's bias there).  Head widths 64 / 128 / 192 / 256 (attn_route): ft_attn_fwd_lens, which reads the
    lengths on the device and skips what lies past them; every other width: mha_fwd's route for the current precision with a byte mask derived
    from lens, followed by mask_rows."""
    B, T, d = x.shape
    nh = int(nheads)
    hd = d // nh
    scale = 1.0 / math.sqrt(hd)
    qkv = H.linear_fwd(x, in_w, in_b)                                   # [B,T,3d]
    route = attn_route(hd, ragged=True)
    if route == 'lens':
        att = H.attn_fwd_lens(qkv, lens, nh, scale)
    else:
        key_pad = (torch.arange(T, device=x.device).unsqueeze(0) >= lens.unsqueeze(1)).to(torch.uint8).contiguous()
        if route == 'fused':
            att = H.attn_fwd(qkv, key_pad, nh, scale, 0.0, 0)[0]
        else:
            att = _attn_unfused(qkv, key_pad, nh, scale, 0.0, 0)[0]
        att = H.mask_rows(att, lens)
    return H.linear_fwd(att, out_w, out_b)


def mha_bwd(tape, dout, in_w, in_b, out_w, out_b, need_dx=True, dx_into=None):
    """-> (dx or None, g_in_w, g_in_b, g_out_w, g_out_b); dx_into: an existing gradient of x that dx is ADDED onto"""
    x, qkv, att, key_pad = tape['x'], tape['qkv'], tape['att'], tape['key_pad']
    nh, hd, scale, p_drop, seed = tape['nh'], tape['hd'], tape['scale'], tape['p'], tape['seed']
    B, T, d = x.shape
    rows = B * T
    dev = x.device
    datt = H.linear_bwd_data(dout, out_w)
    g_ow = emit(out_w, lambda o: H.linear_bwd_weight_raw(dout.data_ptr(), d, att.data_ptr(), d, o, rows, d, d),
                (dout, att))
    g_ob = emit(out_b, lambda o: H.colsum_raw(dout.data_ptr(), d, o, rows, d), (dout,), heavy='light')
    if tape['fused']:
        dqkv = H.attn_bwd(qkv, att, datt, key_pad, tape['lse2'], nh, scale, p_drop, seed)
        g0 = dqkv.data_ptr()
    else:
        P, Pd = tape['P'], tape['Pd']
        q0 = qkv.data_ptr()
        dqkv = torch.empty_like(qkv)
        g0 = dqkv.data_ptr()
        Tp = P.shape[-1]
        dP = torch.empty_like(P)
        # dPd = dAtt_h V_h^T
        _bgemm('nt', datt.data_ptr(), d, T * d, hd, q0 + 2 * d * _F4, 3 * d, T * 3 * d, hd, dP.data_ptr(), Tp,
               nh * T * Tp, T * Tp, T, T, hd, B, nh, dev)
        # dV_h = Pd^T dAtt_h
        _bgemm('tn', Pd.data_ptr(), Tp, nh * T * Tp, T * Tp, datt.data_ptr(), d, T * d, hd, g0 + 2 * d * _F4, 3 * d,
               T * 3 * d, hd, T, hd, T, B, nh, dev, padded=True)
        # dPd -> dS: the dropout mask is re-derived inside the softmax gradient kernel
        _lib.call('ft_softmax_bwd', P.data_ptr(), dP.data_ptr(), B, nh, T, T, Tp, scale, p_drop, seed, H._stream())
        # dQ_h = dS K_h ; dK_h = dS^T Q_h
        _bgemm('nn', dP.data_ptr(), Tp, nh * T * Tp, T * Tp, q0 + d * _F4, 3 * d, T * 3 * d, hd, g0, 3 * d, T * 3 * d,
               hd, T, hd, T, B, nh, dev, padded=True)
        _bgemm('tn', dP.data_ptr(), Tp, nh * T * Tp, T * Tp, q0, 3 * d, T * 3 * d, hd, g0 + d * _F4, 3 * d, T * 3 * d,
               hd, T, hd, T, B, nh, dev, padded=True)
    dx = None
    if need_dx:
        dx = H.linear_bwd_data(dqkv, in_w, dx=dx_into, accumulate=dx_into is not None)
    g_iw = emit(in_w, lambda o: H.linear_bwd_weight_raw(g0, 3 * d, x.data_ptr(), d, o, rows, d, 3 * d), (dqkv, x))
    g_ib = emit(in_b, lambda o: H.colsum_raw(g0, 3 * d, o, rows, 3 * d), (dqkv,), heavy='light')
    return dx, g_iw, g_ib, g_ow, g_ob


class MHAFn(Function):
    """mha_fwd / mha_bwd as one autograd node (the layer-level entry; models run whole transformers through
    TransformerFn)."""

    @staticmethod
    def forward(ctx, x, key_pad, in_w, in_b, out_w, out_b, nheads, p_drop, seed):
        out, ctx.tape = mha_fwd(_c(x), key_pad, in_w, in_b, out_w, out_b, nheads, p_drop, seed)
        ctx.params = (in_w, in_b, out_w, out_b)
        return out

    @staticmethod
    def backward(ctx, dout):
        dx, g_iw, g_ib, g_ow, g_ob = mha_bwd(ctx.tape, _c(dout), *ctx.params, need_dx=ctx.needs_input_grad[0])
        ctx.tape = None
        return dx, None, g_iw, g_ib, g_ow, g_ob, None, None, None


def addln_fwd(x, res, gamma, beta, eps, p=0.0, seed=0):
    """LayerNorm(x + dropout_p(res)) in one pass -> (y, tape); res None: plain LayerNorm"""
    D = x.shape[-1]
    rows = x.numel() // D
    s = torch.empty_like(x) if res is not None else x
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=x.device, dtype=x.dtype)
    rstd = torch.empty(rows, device=x.device, dtype=x.dtype)
    p = float(p) if res is not None else 0.0
    _lib.call('ft_layernorm_fwd', x.data_ptr(), _p(_c(res) if res is not None else None), gamma.data_ptr(),
              beta.data_ptr(), s.data_ptr() if res is not None else None, y.data_ptr(), mean.data_ptr(),
              rstd.data_ptr(), rows, D, float(eps), p, int(seed), H._stream())
    return y, dict(s=s, mean=mean, rstd=rstd, has_res=res is not None, p=p, seed=int(seed))


def addln_bwd(tape, dy, gamma, beta, own_dres=False):
    """-> (dx, dres or None, dgamma, dbeta).  Without dropout the residual branch's gradient IS dx: the same tensor is
    returned twice unless own_dres asks for a copy of its own (a caller that goes on to accumulate into one of them
    while a side-stream weight gradient still reads the other must)."""
    s, mean, rstd = tape['s'], tape['mean'], tape['rstd']
    D = s.shape[-1]
    rows = s.numel() // D
    dx = torch.empty_like(s)
    t = torch.empty_like(s)
    dres = torch.empty_like(s) if tape['has_res'] and (tape['p'] > 0 or own_dres) else None
    _lib.call('ft_layernorm_bwd', dy.data_ptr(), s.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
              dx.data_ptr(), t.data_ptr(), _p(dres), rows, D, tape['p'], tape['seed'], H._stream())
    dg, db = emit([gamma, beta], lambda o: H.colsum2_raw(t.data_ptr(), dy.data_ptr(), D, o[0], o[1], rows, D),
                  (t, dy), heavy='light')
    return dx, ((dres if dres is not None else dx) if tape['has_res'] else None), dg, db


def convbias_fwd(x, w, b, relu):
    """nn.Conv1d(Cin, Cout, k, padding=k//2) with bias (+ ReLU) on channels-last x -> (y, tape)"""
    B, T, Cin = x.shape
    Cout, _, k = w.shape
    wp = H.conv_pack_weight(w)
    y = torch.empty(B, T, Cout, device=x.device, dtype=x.dtype)
    _lib.call('ft_conv1d_bias_fwd', x.data_ptr(), Cin, wp.data_ptr(), b.data_ptr(), y.data_ptr(), Cout, B, T, Cin,
              Cout, k, int(relu), H._stream())
    return y, dict(x=x, wp=wp, y=y if relu else None, relu=bool(relu))


def convbias_bwd(tape, dy, w, b, need_dx=True, dx_into=None):
    """-> (dx or None, dw, db); dx_into: an existing gradient of x that dx is ADDED onto"""
    x, wp, y = tape['x'], tape['wp'], tape['y']
    B, T, Cin = x.shape
    Cout = w.shape[0]
    if tape['relu']:
        g = torch.empty_like(dy)
        _lib.call('ft_relu_bwd', dy.data_ptr(), y.data_ptr(), g.data_ptr(), dy.numel(), H._stream())
        dy = g
    dx = None
    if need_dx:
        dx = dx_into if dx_into is not None else torch.empty_like(x)
        H.conv1d_bwd_data_raw(dy.data_ptr(), Cout, wp, dx, B, T, T, T, dx_into is not None, w=w)
    dw = emit(w, lambda o: H.conv1d_bwd_weight_raw(dy.data_ptr(), Cout, x, o, T, T), (dy, x))
    db = emit(b, lambda o: H.colsum_raw(dy.data_ptr(), Cout, o, B * T, Cout), (dy,), heavy='light')
    return dx, dw, db


class AddLayerNormFn(Function):
    """LayerNorm(x + dropout_p(res))  (FFTBlock: src = norm(src + dropout(src2)), common_layers.py:175-176,181-183) in
    one pass: the dropout of the residual branch uses the same counter-based mask as ops.DropoutFn, applied while the
    rows are normalised (no separate dropout pass forward or backward).  res=None: plain LayerNorm
    (ForwardTransformer.norm, :217)."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, p=0.0, seed=0):
        y, ctx.tape = addln_fwd(_c(x), res, gamma, beta, eps, p, seed)
        ctx.params = (gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, dres, dg, db = addln_bwd(ctx.tape, _c(dy), *ctx.params)
        ctx.tape = None
        return dx, dres, dg, db, None, None, None


class ConvBiasFn(Function):
    """nn.Conv1d(Cin, Cout, k, padding=k//2) with bias (+ ReLU) on channels-last x (FFTBlock conv1/conv2)."""

    @staticmethod
    def forward(ctx, x, w, b, relu):
        y, ctx.tape = convbias_fwd(_c(x), w, b, relu)
        ctx.params = (w, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, dw, db = convbias_bwd(ctx.tape, _c(dy), *ctx.params, need_dx=ctx.needs_input_grad[0])
        ctx.tape = None
        return dx, dw, db, None


def check_posenc_length(T: int, pe: torch.Tensor) -> None:
    """the kernels index pe[t] for t < T: a sequence longer than the `pe` buffer (max_len = 5000 positions) must fail
    like the reference's shape error (common_layers.py:144), not read past the buffer"""
    if T > pe.shape[0] or pe.numel() < T * pe.shape[-1]:
        raise _lib.FtError(f'PositionalEncoding: sequence of {T} positions exceeds the pe buffer ({pe.shape[0]})')


def posenc_fwd(x, pe, scale):
    """x + scale * pe[:T] on contiguous x [B,T,D]: the one place that checks the length and launches ft_posenc_fwd"""
    B, T, D = x.shape
    check_posenc_length(T, pe)
    out = torch.empty_like(x)
    _lib.call('ft_posenc_fwd', x.data_ptr(), pe.data_ptr(), scale.data_ptr(), out.data_ptr(), B, T, D, H._stream())
    return out


def posenc_bwd_scale(dout, pe, scale):
    """gradient of the learnable scale, sum(dout * pe[:T]), emitted like every other parameter gradient"""
    B, T, D = dout.shape

    def dscale(o):
        _lib.call('ft_posenc_bwd_scale', dout.data_ptr(), pe.data_ptr(), o.data_ptr(), B, T, D,
                  *H.scratch('ft_posenc_workspace', device=dout.device), H._stream())

    return emit(scale, dscale, heavy=False)


class PosEncFn(Function):
    """x + scale * pe[:T]  (PositionalEncoding.forward, common_layers.py:143-145)."""

    @staticmethod
    def forward(ctx, x, pe, scale):
        ctx.save_for_backward(pe, scale)
        return posenc_fwd(_c(x), pe, scale)

    @staticmethod
    def backward(ctx, dout):
        pe, scale = ctx.saved_tensors
        dout = _c(dout)
        return dout, None, posenc_bwd_scale(dout, pe, scale)


# ---------------------------------------------------------------------------------------------------
# whole FFTBlocks per C call (include/fwdtaco_hip.h: FtFFTBlock, ft_fft_blocks_fwd / ft_fft_blocks_bwd)
# ---------------------------------------------------------------------------------------------------
import ctypes as _ct

_FP = _ct.c_void_p


class _CBlock(_ct.Structure):
    _fields_ = ([(n, _ct.c_int) for n in ('B', 'T', 'd', 'nheads', 'dfft', 'k1', 'k2')]
                + [(n, _ct.c_float) for n in ('p_drop', 'eps1', 'eps2')]
                + [(n, _ct.c_uint64) for n in ('seed_attn', 'seed_ln1', 'seed_ln2')]
                + [(n, _FP) for n in ('key_pad', 'in_w', 'in_b', 'out_w', 'out_b', 'c1_wp', 'c1_b', 'c2_wp', 'c2_b', 'n1_g',
                                      'n1_b', 'n2_g', 'n2_b', 'in_wT', 'out_wT', 'c1_wpt', 'c2_wpt', 'x', 'qkv', 'att',
                                      'lse2', 'sa', 's1', 'mean1', 'rstd1', 'y1', 'h1', 'h2', 's2', 'mean2', 'rstd2', 'y2')])


class _CGrads(_ct.Structure):
    _fields_ = [(n, _FP) for n in ('dy2', 'dx', 't2', 'd_y1', 'd_h2', 'd_h1', 'g_h1', 't1', 'd_h', 'd_sa', 'datt', 'dqkv',
                                   'g_in_w', 'g_in_b', 'g_out_w', 'g_out_b', 'g_c1_w', 'g_c1_b', 'g_c2_w', 'g_c2_b',
                                   'g_n1_g', 'g_n1_b', 'g_n2_g', 'g_n2_b')]


_sums_streams = {}


def _sums_stream(device) -> 'torch.cuda.Stream':
    key = torch.device(device).index or 0
    if key not in _sums_streams:
        # high priority: twelve small kernels per block -- at default priority they only find free CUs once the other
        # streams' one-wave GEMM grids have drained (the step's join then waited 5 ms for them)
        _sums_streams[key] = torch.cuda.Stream(device=device, priority=-1)
    return _sums_streams[key]


_GRAD_FIELDS = ('g_in_w', 'g_in_b', 'g_out_w', 'g_out_b', 'g_c1_w', 'g_c1_b', 'g_c2_w', 'g_c2_b', 'g_n1_g', 'g_n1_b', 'g_n2_g',
                'g_n2_b')


def _block_params(l: nn.Module):
    """the twelve parameter tensors of an FFTBlock in the order TransformerFn takes them, which is _GRAD_FIELDS' order"""
    a = l.self_attn
    return [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, l.conv1.weight, l.conv1.bias,
            l.conv2.weight, l.conv2.bias, l.norm1.weight, l.norm1.bias, l.norm2.weight, l.norm2.bias]


def _carve(buf: torch.Tensor, sizes):
    """16-byte aligned float sub-buffers of one allocation -> (device addresses, element offsets)"""
    base, off, out, offs = buf.data_ptr(), 0, [], []
    for n in sizes:
        out.append(base + 4 * off)
        offs.append(off)
        off += (n + 3) // 4 * 4
    return out, offs


def _arena(sizes, device):
    return torch.empty(sum((n + 3) // 4 * 4 for n in sizes), device=device, dtype=torch.float32)


def composite_ok(d: int, nheads: int) -> bool:
    """whole blocks per C call: the bf16 mode with the fused attention (head width 64 / 128)"""
    return d % nheads == 0 and attn_route(d // nheads) == 'fused' and os.environ.get('FT_FFT_COMPOSITE', '1') == '1'


def blocks_fwd_composite(h, key_pad, params, nhead, p, eps1, eps2, seeds):
    """every launch of the transformer's FFTBlocks from ONE C call -> (output of the last block, state for the backward)"""
    B, T, d = h.shape
    R = B * T
    n = len(params) // 12
    f = params[4].shape[0]
    k1, k2 = params[4].shape[2], params[6].shape[2]
    sizes = [3 * R * d, R * d, B * nhead * T, R * d, R * d, R, R, R * d, R * f, R * d, R * d, R, R, R * d]
    names = ('qkv', 'att', 'lse2', 'sa', 's1', 'mean1', 'rstd1', 'y1', 'h1', 'h2', 's2', 'mean2', 'rstd2', 'y2')
    blocks = (_CBlock * n)()
    arenas, keep = [], []
    x_ptr = h.data_ptr()
    for i in range(n):
        in_w, in_b, out_w, out_b, c1w, c1b, c2w, c2b, n1g, n1b, n2g, n2b = params[12 * i:12 * i + 12]
        ar = _arena(sizes, h.device)
        arenas.append(ar)
        addr, offs = _carve(ar, sizes)
        ptrs = dict(zip(names, addr))
        y2_off = offs[-1]
        c1p, c2p = H.conv_pack_weight(c1w), H.conv_pack_weight(c2w)
        keep += [c1p, c2p]
        b = blocks[i]
        b.B, b.T, b.d, b.nheads, b.dfft, b.k1, b.k2 = B, T, d, nhead, f, k1, k2
        b.p_drop, b.eps1, b.eps2 = p, eps1, eps2
        b.seed_attn, b.seed_ln1, b.seed_ln2 = seeds[3 * i], seeds[3 * i + 1], seeds[3 * i + 2]
        b.key_pad = _p(key_pad)
        b.in_w, b.in_b, b.out_w, b.out_b = in_w.data_ptr(), in_b.data_ptr(), out_w.data_ptr(), out_b.data_ptr()
        b.c1_wp, b.c1_b, b.c2_wp, b.c2_b = c1p.data_ptr(), c1b.data_ptr(), c2p.data_ptr(), c2b.data_ptr()
        b.n1_g, b.n1_b, b.n2_g, b.n2_b = n1g.data_ptr(), n1b.data_ptr(), n2g.data_ptr(), n2b.data_ptr()
        b.x = x_ptr
        for k_, v_ in ptrs.items():
            setattr(b, k_, v_)
        x_ptr = ptrs['y2']
    _lib.call('ft_fft_blocks_fwd', _ct.byref(blocks), n, H._stream())
    y = arenas[-1][y2_off:y2_off + R * d].view(B, T, d)          # the last block's output, in place
    return y, dict(blocks=blocks, arenas=arenas, keep=keep, h=h, key_pad=key_pad, dims=(B, T, d, f, k1, k2, nhead))


def blocks_bwd_composite(state, dy, params):
    """-> (d wrt the first block's input, list of the 12 * n parameter gradients (None where a gradient sink took them))"""
    blocks = state['blocks']
    B, T, d, f, k1, k2, nhead = state['dims']
    R = B * T
    n = len(params) // 12
    dev = dy.device
    sizes = [R * d, R * d, R * d, R * f, R * f, R * d, R * d, R * d, R * d, 3 * R * d]
    names = ('t2', 'd_y1', 'd_h2', 'd_h1', 'g_h1', 't1', 'd_h', 'd_sa', 'datt', 'dqkv')
    grads = (_CGrads * n)()
    scratch, outs, sunk = [], [None] * (12 * n), []
    sink = installed()
    dy_ptr = dy.data_ptr()
    last_dh = None
    for i in range(n - 1, -1, -1):
        ps = params[12 * i:12 * i + 12]
        b, g = blocks[i], grads[i]
        wit, wot = H.transpose2d(ps[0]), H.transpose2d(ps[2])
        c1t, c2t = H.conv_pack_weight_t(ps[4]), H.conv_pack_weight_t(ps[6])
        scratch += [wit, wot, c1t, c2t]         # (referenced until the launches that read them have been issued AND run)
        b.in_wT, b.out_wT = wit.data_ptr(), wot.data_ptr()
        b.c1_wpt, b.c2_wpt = c1t.data_ptr(), c2t.data_ptr()
        ar = _arena(sizes, dev)
        scratch.append(ar)
        addr, offs = _carve(ar, sizes)
        ptrs = dict(zip(names, addr))
        for k_, v_ in ptrs.items():
            setattr(g, k_, v_)
        g.dy2, g.dx = dy_ptr, ptrs['d_h']
        dy_ptr = ptrs['d_h']
        last_dh = (ar, offs[names.index('d_h')])
        for j, name in enumerate(_GRAD_FIELDS):
            ent = sink.claim(ps[j]) if sink is not None else None
            if ent is not None:                 # (a second emitter of the same parameter would get a fresh tensor)
                sunk.append(ent[0])
                setattr(g, name, ent[1].data_ptr())
            else:
                t = torch.empty_like(ps[j])
                outs[12 * i + j] = t
                setattr(g, name, t.data_ptr())
    side = sink.stream if (sink is not None and sink.stream is not None) else None
    side_raw = side.cuda_stream if side is not None else H._stream()
    # FT_FFT_SUMS_STREAM=1: the blocks' bias / LayerNorm column sums on a stream of their own instead of behind the weight-
    # gradient GEMMs, which finish 1.9 ms after the main stream (lab/steady_segments_fp.py).  Measured: 15.9 -> 17.3 ms per
    # step, at default and at high priority alike -- 240 more small launches on a fourth stream cost more than the tail
    # they remove (profiles/r03_fastpitch_ab.txt).  Off.
    sums = _sums_stream(dev) if side is not None and os.environ.get('FT_FFT_SUMS_STREAM', '0') == '1' else None
    sums_raw = sums.cuda_stream if sums is not None else None
    # three buffers, never shared: the attention's on this stream, the weight gradients' and the sums' named after theirs
    sws = H.scratch('ft_fft_block_sums_workspace', B, T, d, f, device=dev, stream=('sums', sums_raw)) if sums is not None \
        else (None, 0)
    _lib.call('ft_fft_blocks_bwd', _ct.byref(blocks), _ct.byref(grads), n,
              *H.scratch('ft_attn_workspace', B, T, nhead, device=dev),
              *H.scratch('ft_fft_block_wgrad_workspace', B, T, d, f, k1, k2, device=dev, stream=('wgrad', side_raw)),
              *sws, H._stream(), side_raw, sums_raw)
    if sums is not None:
        sink.wrote_on(sums, tell_reducer=True)
    dx = last_dh[0][last_dh[1]:last_dh[1] + R * d].view(B, T, d)     # d wrt the first block's input, in place
    if sink is None:
        dx._ft_keep = (scratch, state['arenas'], state['keep'])       # no sink: everything ran on this stream, in order
    if sink is not None:
        # read by the weight-gradient stream until joined; state['h'] is block 0's input, the operand of the LAST weight
        # gradient issued (its in-projection's): the caller drops `state` as soon as this returns, and a freed `h` is the
        # main stream's to reuse while that GEMM still reads it
        sink.hold((scratch, state['arenas'], state['keep'], dy, state['h'], state['key_pad']))
        if side is not None:
            sink.wrote_on(side)
        if sunk:
            sink.announce(sunk)
    return dx, outs


class TransformerFn(Function):
    """A whole ForwardTransformer (common_layers.py:188-223: positional encoding + dropout, `layers` FFTBlocks, final
    LayerNorm) as ONE autograd node.  Same kernels, same order, same dropout seeds as the per-layer Functions above; what
    goes away is the host side: ~6 autograd nodes per block forward and as many Python backward calls through the
    engine (a FastPitch step was 130 nodes and 14.7 ms of host time for 15 ms of GPU work) -- and the gradient joins of
    the two residual connections, which autograd did with two element-wise adds per block, are now the accumulate
    epilogues of the data-gradient GEMMs that produce the second addend.
    args: x, key_pad, pe, pe_scale, norm_g, norm_b, then 12 tensors per block (in_w, in_b, out_w, out_b, conv1 w, b,
    conv2 w, b, norm1 g, b, norm2 g, b); cfg = (nhead, p_block, p_posenc, training, eps1, eps2, eps_final)."""

    @staticmethod
    def forward(ctx, x, key_pad, pe, pe_scale, norm_g, norm_b, cfg, *params):
        nhead, p_blk, p_pe, training, eps1, eps2, eps_f = cfg
        x = _c(x)
        D = x.shape[2]
        h = posenc_fwd(x, pe, pe_scale)
        pe_seed = 0
        if training and p_pe > 0:
            pe_seed = _seed()
            h = H.dropout(h, p_pe, pe_seed)
        p = p_blk if training else 0.0
        tapes = []
        ctx.comp = None
        if composite_ok(D, nhead) and len(params) >= 12:
            seeds = [(_seed() if p > 0 else 0) for _ in range(3 * (len(params) // 12))]
            h, ctx.comp = blocks_fwd_composite(h, key_pad, params, nhead, p, eps1, eps2, seeds)
            params_loop = ()
        else:
            params_loop = params
        for i in range(len(params_loop) // 12):
            in_w, in_b, out_w, out_b, c1w, c1b, c2w, c2b, n1g, n1b, n2g, n2b = params[12 * i:12 * i + 12]
            s0 = _seed() if p > 0 else 0
            sa, t_mha = mha_fwd(h, key_pad, in_w, in_b, out_w, out_b, nhead, p, s0)
            y1, t_n1 = addln_fwd(h, sa, n1g, n1b, eps1, p, _seed() if p > 0 else 0)
            h1, t_c1 = convbias_fwd(y1, c1w, c1b, True)
            h2, t_c2 = convbias_fwd(h1, c2w, c2b, False)
            h, t_n2 = addln_fwd(y1, h2, n2g, n2b, eps2, p, _seed() if p > 0 else 0)
            tapes.append((t_mha, t_n1, t_c1, t_c2, t_n2))
        y, t_f = addln_fwd(h, None, norm_g, norm_b, eps_f)
        ctx.tapes, ctx.t_f, ctx.params = tapes, t_f, params
        ctx.head = (pe, pe_scale, norm_g, norm_b, p_pe if training else 0.0, pe_seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        pe, pe_scale, norm_g, norm_b, p_pe, pe_seed = ctx.head
        params = ctx.params
        grads = [None] * len(params)
        d, _, g_ng, g_nb = addln_bwd(ctx.t_f, _c(dy), norm_g, norm_b)
        if ctx.comp is not None:
            d, grads = blocks_bwd_composite(ctx.comp, d, params)
            ctx.comp = None
        for i in range(len(ctx.tapes) - 1, -1, -1):
            in_w, in_b, out_w, out_b, c1w, c1b, c2w, c2b, n1g, n1b, n2g, n2b = params[12 * i:12 * i + 12]
            t_mha, t_n1, t_c1, t_c2, t_n2 = ctx.tapes[i]
            with batched_side_launches():       # the block's six weight / six bias gradients: one side-stream hand-over
                d_y1, d_h2, g_n2g, g_n2b = addln_bwd(t_n2, d, n2g, n2b, own_dres=True)
                d_h1, g_c2w, g_c2b = convbias_bwd(t_c2, d_h2, c2w, c2b)
                d_y1, g_c1w, g_c1b = convbias_bwd(t_c1, d_h1, c1w, c1b, dx_into=d_y1)          # + the residual path
                d_h, d_sa, g_n1g, g_n1b = addln_bwd(t_n1, d_y1, n1g, n1b, own_dres=True)
                d, g_iw, g_ib, g_ow, g_ob = mha_bwd(t_mha, d_sa, in_w, in_b, out_w, out_b, dx_into=d_h)   # + the residual path
            grads[12 * i:12 * i + 12] = [g_iw, g_ib, g_ow, g_ob, g_c1w, g_c1b, g_c2w, g_c2b, g_n1g, g_n1b, g_n2g, g_n2b]
        ctx.tapes = None
        if p_pe > 0:
            d = H.dropout(d, p_pe, pe_seed)
        g_scale = posenc_bwd_scale(d, pe, pe_scale)
        return (d if ctx.needs_input_grad[0] else None, None, None, g_scale, g_ng, g_nb, None, *grads)


# ---------------------------------------------------------------------------------------------------
class PositionalEncoding(nn.Module):
    """common_layers.py:127-145 (buffer `pe` [max_len,1,d] and learnable scalar `scale` kept for the state_dict)."""

    def __init__(self, d_model: int, dropout=0.1, max_len=5000) -> None:
        super().__init__()
        self.p = dropout
        self.scale = nn.Parameter(torch.ones(1))
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer('pe', pe.unsqueeze(0).transpose(0, 1))

    def forward(self, x: torch.Tensor) -> torch.Tensor:            # x [B,T,d]
        x = PosEncFn.apply(x, self.pe, self.scale)
        return _dropout(x, self.p, self.training)


class FFTBlock(nn.Module):
    """common_layers.py:148-185 on batch-major [B,T,d]."""

    def __init__(self, d_model: int, nhead: int, conv1_kernel: int, conv2_kernel: int, d_fft: int,
                 dropout: float = 0.1):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.conv1 = nn.Conv1d(in_channels=d_model, out_channels=d_fft, kernel_size=conv1_kernel, stride=1,
                               padding=conv1_kernel // 2)
        self.conv2 = nn.Conv1d(in_channels=d_fft, out_channels=d_model, kernel_size=conv2_kernel, stride=1,
                               padding=conv2_kernel // 2)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.nhead = nhead
        self.p = dropout

    def forward(self, src: torch.Tensor, key_pad: Optional[torch.Tensor] = None) -> torch.Tensor:
        a = self.self_attn
        p = self.p if self.training else 0.0
        seed = _seed() if p > 0 else 0
        src2 = MHAFn.apply(src, key_pad, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
                           self.nhead, p, seed)
        # the two F.dropout of the residual branches (common_layers.py:175,182) are fused into the LayerNorm kernels
        src = AddLayerNormFn.apply(src, src2, self.norm1.weight, self.norm1.bias, self.norm1.eps, p,
                                   _seed() if p > 0 else 0)
        src2 = ConvBiasFn.apply(src, self.conv1.weight, self.conv1.bias, True)
        src2 = ConvBiasFn.apply(src2, self.conv2.weight, self.conv2.bias, False)
        return AddLayerNormFn.apply(src, src2, self.norm2.weight, self.norm2.bias, self.norm2.eps, p,
                                    _seed() if p > 0 else 0)

    def forward_lens(self, src: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """eval forward of a ragged batch (torch.no_grad): no valid row reads a row at t >= lens[b].  The attention
        guarantees that itself; the k > 1 convolutions need their input zero there, so both LayerNorms store zeros past
        the item's length (a LayerNorm would turn a zero row into its beta) and both convolutions mask their output.
        -> [B,T,d], exactly 0 at t >= lens[b]"""
        a = self.self_attn
        src2 = mha_fwd_lens(src, lens, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, self.nhead)
        src = H.add_layernorm_fwd_lens(src, src2, self.norm1.weight, self.norm1.bias, lens, self.norm1.eps)
        h = H.conv1d_bias_fwd_lens(src, H.conv_pack_weight(self.conv1.weight), self.conv1.bias, True, lens)
        h = H.conv1d_bias_fwd_lens(h, H.conv_pack_weight(self.conv2.weight), self.conv2.bias, False, lens)
        return H.add_layernorm_fwd_lens(src, h, self.norm2.weight, self.norm2.bias, lens, self.norm2.eps)


class ForwardTransformer(nn.Module):
    """common_layers.py:188-223; x [B,T,d] -> [B,T,d].  Like the reference, every layer is a deepcopy of ONE
    initialised FFTBlock, so all layers start from identical weights."""

    def __init__(self, d_model: int, d_fft: int, layers: int, heads: int, conv1_kernel: int, conv2_kernel: int,
                 dropout: float = 0.1) -> None:
        super().__init__()
        self.d_model = d_model
        self.pos_encoder = PositionalEncoding(d_model, dropout)
        encoder_layer = FFTBlock(d_model=d_model, nhead=heads, d_fft=d_fft, conv1_kernel=conv1_kernel,
                                 conv2_kernel=conv2_kernel, dropout=dropout)
        encoder_norm = nn.LayerNorm(d_model)
        self.layers = nn.ModuleList([copy.deepcopy(encoder_layer) for _ in range(layers)])
        self.norm = encoder_norm

    def forward(self, x: torch.Tensor, src_pad_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        key_pad = None
        if src_pad_mask is not None:
            key_pad = src_pad_mask.to(torch.uint8).contiguous()
        # One autograd node per transformer (its FFTBlocks issued from C) in the bf16 mode, where the step was bound by the
        # host; one node per operation in the fp32 mode, which is GPU-bound either way and overlaps better when every
        # weight gradient is side-launched the moment its node runs (25.0 vs 25.5 ms).  FT_TRANSFORMER_NODE=0 / 1 overrides.
        node = os.environ.get('FT_TRANSFORMER_NODE')
        if (node != '1') if node is not None else (H.gemm_precision_mode() != 'bf16'):
            x = self.pos_encoder(x)
            for layer in self.layers:
                x = layer(x, key_pad)
            return AddLayerNormFn.apply(x, None, self.norm.weight, self.norm.bias, self.norm.eps)
        flat = [t for l in self.layers for t in _block_params(l)]
        l0 = self.layers[0]
        cfg = (l0.nhead, l0.p, self.pos_encoder.p, self.training, l0.norm1.eps, l0.norm2.eps, self.norm.eps)
        return TransformerFn.apply(x, key_pad, self.pos_encoder.pe, self.pos_encoder.scale, self.norm.weight,
                                   self.norm.bias, cfg, *flat)

    def forward_lens(self, x: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """eval forward of a ragged batch, operation by operation in both precisions (the C-issued composite is the
        training path): x [B,T,d], lens int64 [B] on the device -> [B,T,d], exactly 0 at t >= lens[b].  Rows of x at
        t >= lens[b] are never read into a valid row (with the fused attention kernel they may even hold NaN)."""
        h = posenc_fwd(_c(x), self.pos_encoder.pe, self.pos_encoder.scale)
        for layer in self.layers:
            h = layer.forward_lens(h, lens)
        return H.add_layernorm_fwd_lens(h, None, self.norm.weight, self.norm.bias, lens, self.norm.eps)


class SeriesPredictor(nn.Module):
    """fast_pitch.py:14-41"""

    def __init__(self, num_chars: int, d_model: int, n_heads: int, d_fft: int, layers: int, conv1_kernel: int,
                 conv2_kernel: int, dropout=0.1):
        super().__init__()
        self.embedding = nn.Embedding(num_chars, d_model)
        self.transformer = ForwardTransformer(heads=n_heads, dropout=dropout, d_model=d_model, d_fft=d_fft,
                                              conv1_kernel=conv1_kernel, conv2_kernel=conv2_kernel, layers=layers)
        self.lin = nn.Linear(d_model, 1)

    def forward(self, x: torch.Tensor, src_pad_mask: Optional[torch.Tensor] = None, alpha: float = 1.0):
        return transformer_predict(self, predictor_front(x, self.embedding), src_pad_mask, alpha)

    def forward_lens(self, x: torch.Tensor, lens: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
        """eval forward of a ragged batch: tokens at t >= lens[b] are ignored, the result [B,T,1] is zero there"""
        y = self.transformer.forward_lens(H.embedding_fwd_lens(x, lens, self.embedding.weight), lens)
        return H.mask_rows(predictor_tail(y, self.lin, alpha), lens)            # (the Linear's bias)


def transformer_predict(pred: nn.Module, x: torch.Tensor, src_pad_mask: Optional[torch.Tensor], alpha: float):
    """ForwardTransformer -> Linear (/ alpha) of the transformer series predictors, on the output of
    base.predictor_front"""
    return predictor_tail(pred.transformer(x, src_pad_mask=src_pad_mask), pred.lin, alpha)


class FastPitch(AcousticModel):
    """Drop-in for models/fast_pitch.py:44-235.  `matmul_dtype` (base.AcousticModel) selects fp32 or bf16 matmuls."""
    config_key = 'fast_pitch'

    def __init__(self, num_chars: int,
                 durpred_dropout: float, durpred_d_model: int, durpred_n_heads: int, durpred_layers: int,
                 durpred_d_fft: int,
                 pitch_dropout: float, pitch_d_model: int, pitch_n_heads: int, pitch_layers: int, pitch_d_fft: int,
                 energy_dropout: float, energy_d_model: int, energy_n_heads: int, energy_layers: int,
                 energy_d_fft: int,
                 pitch_strength: float, energy_strength: float, d_model: int, conv1_kernel: int, conv2_kernel: int,
                 prenet_layers: int, prenet_heads: int, prenet_fft: int, prenet_dropout: float,
                 postnet_layers: int, postnet_heads: int, postnet_fft: int, postnet_dropout: float,
                 n_mels: int, padding_value=PAD_VALUE):
        super().__init__()
        self.padding_value = padding_value
        self.lr = LengthRegulator()
        self.dur_pred = SeriesPredictor(num_chars=num_chars, d_model=durpred_d_model, n_heads=durpred_n_heads,
                                        layers=durpred_layers, d_fft=durpred_d_fft, conv1_kernel=conv1_kernel,
                                        conv2_kernel=conv2_kernel, dropout=durpred_dropout)
        self.pitch_pred = SeriesPredictor(num_chars=num_chars, d_model=pitch_d_model, n_heads=pitch_n_heads,
                                          layers=pitch_layers, d_fft=pitch_d_fft, conv1_kernel=conv1_kernel,
                                          conv2_kernel=conv2_kernel, dropout=pitch_dropout)
        self.energy_pred = SeriesPredictor(num_chars=num_chars, d_model=energy_d_model, n_heads=energy_n_heads,
                                           layers=energy_layers, d_fft=energy_d_fft, conv1_kernel=conv1_kernel,
                                           conv2_kernel=conv2_kernel, dropout=energy_dropout)
        self.embedding = nn.Embedding(num_embeddings=num_chars, embedding_dim=d_model)
        self.prenet = ForwardTransformer(heads=prenet_heads, dropout=prenet_dropout, conv1_kernel=conv1_kernel,
                                         conv2_kernel=conv2_kernel, d_model=d_model, d_fft=prenet_fft,
                                         layers=prenet_layers)
        self.postnet = ForwardTransformer(heads=postnet_heads, dropout=postnet_dropout, conv1_kernel=conv1_kernel,
                                          conv2_kernel=conv2_kernel, d_model=d_model, d_fft=postnet_fft,
                                          layers=postnet_layers)
        self.lin = nn.Linear(d_model, n_mels)
        self.register_buffer('step', torch.zeros(1, dtype=torch.long))
        self.pitch_strength = pitch_strength
        self.energy_strength = energy_strength
        self.pitch_proj = nn.Conv1d(1, d_model, kernel_size=3, padding=1)
        self.energy_proj = nn.Conv1d(1, d_model, kernel_size=3, padding=1)

    def _mel(self, x_idx, tok_mask, dur, pitch, energy, frame_lens: Optional[torch.Tensor]):
        x = ops.EmbeddingFn.apply(x_idx, self.embedding.weight)
        x = self.prenet(x, src_pad_mask=tok_mask)
        x = self._cond_add(x, pitch, energy, False)
        x = self.lr(x, dur)
        frame_mask = None
        if frame_lens is not None:          # fast_pitch.py:152-154
            T = x.shape[1]
            frame_mask = torch.arange(T, device=x.device).unsqueeze(0) >= frame_lens.unsqueeze(1)
        x = self.postnet(x, src_pad_mask=frame_mask)
        return ops.LinearFn.apply(x, self.lin.weight, self.lin.bias)           # [B,T,n_mels]

    @precision_scoped
    def forward(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        x = batch['x']
        mel = batch['mel']
        dur = batch['dur']
        mel_lens = batch['mel_len']
        self._begin_forward(x)
        len_mask = x == 0                                                       # make_token_len_mask

        def predict():      # in the order that fixes the dropout seed sequence: dur, pitch, energy
            dur_hat = self.dur_pred(x, src_pad_mask=len_mask).squeeze(-1)
            pitch_hat = self.pitch_pred(x, src_pad_mask=len_mask).transpose(1, 2)
            energy_hat = self.energy_pred(x, src_pad_mask=len_mask).transpose(1, 2)
            return {'dur': dur_hat, 'pitch': pitch_hat, 'energy': energy_hat}

        # the three token-side predictors only feed the losses in training (fast_pitch.py:129-131 vs :133-150): side HIP
        # stream, concurrently with the frame-side trunk (autograd replays their backward on the same stream)
        fork = self._fork_predictors(x.device, predict)
        mel_cl = self._mel(x, len_mask, dur, batch['pitch'], batch['energy'],
                           mel_lens.to(device=x.device, dtype=torch.long))
        x_mel = ops.TransposePadFn.apply(mel_cl, mel.size(2), self.padding_value)
        return {'mel': x_mel, 'mel_post': x_mel, **self._join_predictors(fork)}

    @precision_scoped
    def generate(self, x: torch.Tensor, alpha=1.0,
                 pitch_function: Callable[[torch.Tensor], torch.Tensor] = lambda x: x,
                 energy_function: Callable[[torch.Tensor], torch.Tensor] = lambda x: x) -> Dict[str, torch.Tensor]:
        self.eval()
        with torch.no_grad():
            self._require_device(x)
            B = x.shape[0]
            # NB (reference quirk, fast_pitch.py:174-180): the predictors run WITHOUT a padding mask here
            dur_hat = self.dur_pred(x, alpha=alpha).squeeze(2)
            if torch.sum(dur_hat.long()) <= 0:
                torch.fill_(dur_hat, value=2.)
            pitch_hat = pitch_function(self.pitch_pred(x).transpose(1, 2))
            energy_hat = energy_function(self.energy_pred(x).transpose(1, 2))
            dur_in = dur_hat.contiguous()
            mel_cl = self._mel(x, x == 0, dur_in, pitch_hat.reshape(B, -1).contiguous(),
                               energy_hat.reshape(B, -1).contiguous(), None)
            m = H.transpose_pad_fwd(mel_cl, mel_cl.shape[1], 0.0)
            return {'mel': m, 'mel_post': m, 'dur': dur_in, 'pitch': pitch_hat, 'energy': energy_hat}

    checks_tokens = True

    @precision_scoped
    def generate_batch(self, x: torch.Tensor, x_len: torch.Tensor, alpha=1.0,
                       pitch_function: Callable[[torch.Tensor], torch.Tensor] = lambda p: p,
                       energy_function: Callable[[torch.Tensor], torch.Tensor] = lambda e: e) -> Dict[str, torch.Tensor]:
        """base.AcousticModel.generate_batch, the whole call under the model's `matmul_dtype`"""
        return super().generate_batch(x, x_len, alpha, pitch_function, energy_function)

    def _ragged_prenet(self, x, xl):
        return self.prenet.forward_lens(H.embedding_fwd_lens(x, xl, self.embedding.weight), xl)

    def _ragged_regulate(self, h, pred):
        h = self._cond_add(h, pred['pitch'], pred['energy'], False)
        return self.lr(h, pred['dur'])                                    # zero rows at t >= mel_len[b]; syncs to size Tm

    def _ragged_finish(self, h, mel_len):
        h = self.postnet.forward_lens(h, mel_len)
        mel = ops.LinearFn.apply(h, self.lin.weight, self.lin.bias)       # [B,Tm,n_mels]
        m = H.transpose_pad_lens_fwd(mel, mel_len, mel.shape[1], float(self.padding_value))
        return m, m                                                       # one tensor, as in generate
