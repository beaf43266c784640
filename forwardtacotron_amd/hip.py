"""Thin tensor-level wrappers over the C ABI (include/fwdtaco_hip.h).

torch is used here only as the owner of device memory and of the HIP stream; every computation is a
hand-written gfx950 kernel behind libfwdtaco_hip.so.  All functions require contiguous fp32 CUDA(HIP)
tensors and raise if handed anything else -- there is no fallback path.
"""
import contextlib
import ctypes
import os
from typing import List, Optional, Sequence, Union

import torch

from . import _lib

c_void_p = ctypes.c_void_p


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_cur_device = getattr(torch._C, '_cuda_getDevice', None)


def _stream():
    """hipStream_t of torch's current stream on the current device.  Goes straight to the C binding: the public
    `torch.cuda.current_stream()` resolves the device through `torch.cuda.is_available()`, i.e. a device-count
    query (~18 us on this stack) per call -- at ~300 launches per step that alone made the FastPitch step host-bound."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, name: str, dtype=torch.float32):
    if not t.is_cuda:
        raise _lib.FtError(f'{name}: expected a device tensor (the HIP path has no CPU fallback)')
    if t.dtype != dtype:
        raise _lib.FtError(f'{name}: expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise _lib.FtError(f'{name}: expected a contiguous tensor')
    return t


_workspaces = {}


def workspace(nbytes: int, device, stream=None) -> torch.Tensor:
    """Grow-only scratch buffer per (device, stream): kernels of one stream run in order, so they can share
    it; concurrent streams (the predictors' side stream) get their own.  stream: the raw stream the buffer is for (or
    any hashable that names a buffer of its own next to that stream's), default torch's current stream."""
    key = (torch.device(device).index or 0, _stream() if stream is None else stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def scratch(query_name: str, *dims, device, stream=None):
    """(address, bytes) of the stream's workspace, grown to what the library's size query `query_name` answers for the
    integers `dims`: the two scratch arguments of the entry point the query belongs to"""
    buf = workspace(_lib.query(query_name, *dims), device, stream)
    return buf.data_ptr(), buf.numel()


def _ptr_array(ts: Sequence[Optional[torch.Tensor]]):
    arr = (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])
    return arr


# ---------------------------------------------------------------------------------------------------
# matmul precision (process-wide switch of the library, include/fwdtaco_hip.h: ft_set_gemm_precision)
# ---------------------------------------------------------------------------------------------------
_PRECISIONS = {'fp32': 0, 'bf16': 1}
_precision_now = 'fp32'


def gemm_precision_mode() -> str:
    """the mode set_gemm_precision last installed"""
    return _precision_now


def set_gemm_precision(mode: str) -> str:
    """'fp32' (default: fp32-exact products) or 'bf16' (operands rounded to bf16, one bf16 MFMA per product, fp32
    accumulation and outputs); returns the previous mode"""
    if mode not in _PRECISIONS:
        raise _lib.FtError(f"gemm precision must be 'fp32' or 'bf16', got {mode!r}")
    global _precision_now
    old = _lib.lib().ft_set_gemm_precision(_PRECISIONS[mode])
    _precision_now = mode
    return 'bf16' if old else 'fp32'


@contextlib.contextmanager
def gemm_precision(mode: str):
    old = set_gemm_precision(mode)
    try:
        yield
    finally:
        set_gemm_precision(old)


# names of ft_gemm_variant_counts' entries, in the ABI's order (include/fwdtaco_hip.h)
GEMM_VARIANTS = (
    'rows_f32_64_nt_fast', 'rows_f32_64_nt_slow', 'rows_f32_64_nn_fast', 'rows_f32_64_nn_slow',
    'rows_f32_128_nt_fast', 'rows_f32_128_nt_slow', 'rows_f32_128_nn_fast', 'rows_f32_128_nn_slow',
    'rows_b3_64', 'rows_b3_128', 'rows_b3p', 'rows_b3p_ksplit',
    'tn_f32_64_fast', 'tn_f32_64_slow', 'tn_f32_128_fast', 'tn_f32_128_slow',
    'tn_b3_64', 'tn_b3_128', 'tn_b3p')


def gemm_variant_counts() -> dict:
    """{variant name: launches since the library loaded} -- which kernel the GEMM launchers dispatched (host counters)"""
    n = len(GEMM_VARIANTS)
    arr = (ctypes.c_long * n)()
    if _lib.query('ft_gemm_variant_counts', ctypes.cast(arr, c_void_p), n) != n:
        raise _lib.FtError('ft_gemm_variant_counts: the library knows another variant list than hip.GEMM_VARIANTS')
    return dict(zip(GEMM_VARIANTS, (int(v) for v in arr)))


# ---------------------------------------------------------------------------------------------------
# fused attention (bf16 mode)
# ---------------------------------------------------------------------------------------------------
def attn_fwd(qkv: torch.Tensor, key_pad: Optional[torch.Tensor], nheads: int, scale: float, p_drop: float, seed: int):
    """qkv [B,T,3d] -> (att [B,T,d], lse2 [B,nheads,T]); include/fwdtaco_hip.h: ft_attn_fwd"""
    _chk(qkv, 'qkv')
    B, T, d3 = qkv.shape
    d = d3 // 3
    att = torch.empty(B, T, d, device=qkv.device, dtype=qkv.dtype)
    lse2 = torch.empty(B, nheads, T, device=qkv.device, dtype=qkv.dtype)
    _lib.call('ft_attn_fwd', _p(qkv), _p(key_pad), _p(att), _p(lse2), B, T, nheads, d // nheads, float(scale),
              float(p_drop), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream())
    return att, lse2


def attn_fwd_lens(qkv: torch.Tensor, lens: torch.Tensor, nheads: int, scale: float) -> torch.Tensor:
    """Inference attention of a ragged batch: qkv [B,T,3d], lens int64 [B] (device) -> att [B,T,d] with rows t < lens[b]
    attending to keys < lens[b] and rows t >= lens[b] exactly 0 (qkv is not read there).  The precision is
    gemm_precision_mode()'s: bf16 = ft_attn_fwd's arithmetic, fp32 = fp32-exact products.  Head width 64, 128, 192 or 256
    (include/fwdtaco_hip.h: ft_attn_fwd_lens)."""
    _chk(qkv, 'qkv'); _chk(lens, 'lens', torch.int64)
    B, T, d3 = qkv.shape
    d = d3 // 3
    assert lens.numel() == B
    att = torch.empty(B, T, d, device=qkv.device, dtype=qkv.dtype)
    _lib.call('ft_attn_fwd_lens', _p(qkv), _p(lens), _p(att), B, T, nheads, d // nheads, float(scale),
              int(gemm_precision_mode() == 'bf16'), _stream())
    return att


def attn_bwd(qkv, att, datt, key_pad, lse2, nheads: int, scale: float, p_drop: float, seed: int) -> torch.Tensor:
    _chk(datt, 'datt')
    B, T, d3 = qkv.shape
    d = d3 // 3
    dqkv = torch.empty_like(qkv)
    _lib.call('ft_attn_bwd', _p(qkv), _p(att), _p(datt), _p(key_pad), _p(lse2), _p(dqkv), B, T, nheads, d // nheads,
              float(scale), float(p_drop), int(seed) & 0xFFFFFFFFFFFFFFFF,
              *scratch('ft_attn_workspace', B, T, nheads, device=qkv.device), _stream())
    return dqkv


# ---------------------------------------------------------------------------------------------------
# linear
# ---------------------------------------------------------------------------------------------------
def linear_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False,
               out: Optional[torch.Tensor] = None, x_tm_B: int = 0, y_tm_B: int = 0) -> torch.Tensor:
    """x [..., in] , w [out, in] -> [..., out].  x_tm_B / y_tm_B > 0: that side is time-major [T,B,*]
    (see include/fwdtaco_hip.h, "Row layouts"); a layout change swaps the two leading dims of the result."""
    _chk(x, 'x'); _chk(w, 'w')
    in_f = x.shape[-1]
    rows = x.numel() // max(in_f, 1) if in_f else 0
    out_f = w.shape[0]
    assert w.shape[1] == in_f
    if out is not None:
        y = out
    elif bool(x_tm_B) != bool(y_tm_B):
        Bq = x_tm_B or y_tm_B
        lead = (rows // Bq, Bq) if y_tm_B else (Bq, rows // Bq)
        y = torch.empty(*lead, out_f, device=x.device, dtype=x.dtype)
    else:
        y = torch.empty(*x.shape[:-1], out_f, device=x.device, dtype=x.dtype)
    _lib.call('ft_linear_fwd', _p(x), in_f, _p(w), _p(bias), _p(y), out_f, rows, in_f, out_f, int(relu), 0,
              x_tm_B, y_tm_B, _stream())
    return y


def linear_multi_fwd(x: torch.Tensor, ws: List[torch.Tensor], biases: Optional[List[Optional[torch.Tensor]]],
                     relu: bool = False, y_tm_B: int = 0, as_rows: int = 0) -> torch.Tensor:
    """Several Linear layers on one (batch-major) input, outputs concatenated along the last dim (one launch).
    y_tm_B > 0: x is [B,T,in] and the result is written time-major [T,B,sum(out)]."""
    _chk(x, 'x')
    in_f = x.shape[-1]
    rows = x.numel() // max(in_f, 1)
    outs = [int(w.shape[0]) for w in ws]
    offs = [sum(outs[:i]) for i in range(len(outs))]
    lead = (rows // y_tm_B, y_tm_B) if y_tm_B else tuple(x.shape[:-1])
    y = torch.empty(*lead, sum(outs), device=x.device, dtype=x.dtype)
    n = len(ws)
    wa = _ptr_array(ws)
    ba = _ptr_array(biases) if biases is not None else None
    oa = (ctypes.c_int * n)(*offs)
    fa = (ctypes.c_int * n)(*outs)
    if as_rows:         # rounded like a launch over as_rows rows (ft_linear_multi_fwd_as)
        assert not relu and not y_tm_B
        _lib.call('ft_linear_multi_fwd_as', _p(x), in_f, n, ctypes.cast(wa, c_void_p),
                  ctypes.cast(ba, c_void_p) if ba is not None else None, _p(y), sum(outs),
                  ctypes.cast(oa, c_void_p), ctypes.cast(fa, c_void_p), rows, in_f, max(int(as_rows), 1), _stream())
        return y
    _lib.call('ft_linear_multi_fwd', _p(x), in_f, n, ctypes.cast(wa, c_void_p),
              ctypes.cast(ba, c_void_p) if ba is not None else None, _p(y), sum(outs),
              ctypes.cast(oa, c_void_p), ctypes.cast(fa, c_void_p), rows, in_f, int(relu), 0, y_tm_B, _stream())
    return y


# every batch-independent GEMM is rounded like a launch over this many rows (the 128 x 128 tile), whatever the batch holds
AS_ROWS = 1 << 20
_as_operands = {}


def linear_fwd_as(x: torch.Tensor, ldx: int, w: torch.Tensor, rows: int, in_f: int, alloc=torch.empty) -> torch.Tensor:
    """y [rows, out_f] = x (read with a row stride of ldx floats, so rows may overlap) * w^T, w [out_f, in_f], on the
    kernel a launch over AS_ROWS rows takes (ft_linear_multi_fwd_as with one weight): the kernel, and with it the
    rounding, does not depend on `rows`, so a row alone gives the bits it gives inside any batch.  The operand arrays
    are a pure function of (w.data_ptr(), out_f) and are kept per such pair."""
    out_f = int(w.shape[0])
    ops = _as_operands.get((w.data_ptr(), out_f))
    if ops is None:
        arrs = (_ptr_array([w]), (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(out_f))
        ops = _as_operands[(w.data_ptr(), out_f)] = tuple(ctypes.cast(a, c_void_p) for a in arrs) + (arrs,)
    y = alloc(rows, out_f, dtype=torch.float32, device=x.device)
    _lib.call('ft_linear_multi_fwd_as', x.data_ptr(), ldx, 1, ops[0], None, y.data_ptr(), out_f, ops[1], ops[2], rows, in_f,
              AS_ROWS, _stream())
    return y


# Data gradients contract over the OUTPUT features, which are the slow index of torch's [out,in] weights.  The
# bf16-split MFMA kernel wants the contraction index contiguous in both operands, so the (small) weight is transposed
# first and the product runs in the NT form; NT_GRADS = False keeps the [K][N] form on the f32 MFMA kernel.
NT_GRADS = True


def _wt(w: torch.Tensor):
    """(pointer-holder tensor, flag) of the weight operand of a data gradient"""
    if NT_GRADS and w.shape[0] % 4 == 0:
        return transpose2d(w), 1
    return w, 0


def linear_bwd_data(dy: torch.Tensor, w: torch.Tensor, dx: Optional[torch.Tensor] = None, accumulate: bool = False,
                    dy_tm_B: int = 0, dx_tm_B: int = 0) -> torch.Tensor:
    """dx = dy @ w ; *_tm_B > 0: that side is time-major."""
    _chk(w, 'w'); _chk(dy, 'dy')
    out_f = dy.shape[-1]
    in_f = w.shape[1]
    rows = dy.numel() // max(out_f, 1)
    if dx is None:
        if bool(dy_tm_B) != bool(dx_tm_B):
            Bq = dy_tm_B or dx_tm_B
            lead = (rows // Bq, Bq) if dx_tm_B else (Bq, rows // Bq)
        else:
            lead = tuple(dy.shape[:-1])
        dx = torch.empty(*lead, in_f, device=dy.device, dtype=dy.dtype)
    wt, flag = _wt(w)
    _lib.call('ft_linear_bwd_data', _p(dy), out_f, _p(wt), _p(dx), in_f, rows, in_f, out_f, int(accumulate),
              dy_tm_B, dx_tm_B, flag, _stream())
    return dx


def linear_bwd_data_raw(dy_ptr: int, lddy: int, w: torch.Tensor, dx: torch.Tensor, rows: int, out_f: int,
                        accumulate: bool, dy_tm_B: int = 0, dx_tm_B: int = 0) -> None:
    in_f = w.shape[1]
    wt, flag = _wt(w)
    _lib.call('ft_linear_bwd_data', dy_ptr, lddy, _p(wt), _p(dx), in_f, rows, in_f, out_f, int(accumulate),
              dy_tm_B, dx_tm_B, flag, _stream())


def linear_bwd_data_multi(dy_ptrs: Sequence[int], lddy: int, ws: Sequence[torch.Tensor], dx: torch.Tensor, rows: int,
                          out_f: int, accumulate: bool = False, dy_tm_B: int = 0, dx_tm_B: int = 0) -> None:
    """dx (+)= sum_i dy_i @ w_i in one chained launch (dy_i given as raw device addresses, common row stride)"""
    n = len(ws)
    in_f = ws[0].shape[1]
    da = (ctypes.c_void_p * n)(*[int(p) for p in dy_ptrs])
    flag = 1 if NT_GRADS and all(w.shape[0] % 4 == 0 for w in ws) else 0
    wts = [transpose2d(w) for w in ws] if flag else list(ws)
    wa = _ptr_array(wts)
    nbytes = _lib.lib().ft_linear_bwd_data_multi_workspace(n, rows, in_f, out_f, _stream()) if flag else 0
    if nbytes:          # few output tiles, long contraction: split-K (scratch from the stream's workspace)
        ws = workspace(nbytes, dx.device)
        _lib.call('ft_linear_bwd_data_multi_ws', n, ctypes.cast(da, c_void_p), lddy, ctypes.cast(wa, c_void_p), _p(dx),
                  in_f, rows, in_f, out_f, int(accumulate), dy_tm_B, dx_tm_B, flag, _p(ws), ws.numel(), _stream())
        return
    _lib.call('ft_linear_bwd_data_multi', n, ctypes.cast(da, c_void_p), lddy, ctypes.cast(wa, c_void_p), _p(dx), in_f,
              rows, in_f, out_f, int(accumulate), dy_tm_B, dx_tm_B, flag, _stream())


def linear_bwd_weight_raw(dy_ptr: int, lddy: int, x_ptr: int, ldx: int, dw: torch.Tensor, rows: int, in_f: int,
                          out_f: int, B: int = 1, T: int = 0, x_shift: int = 0, accumulate: bool = False,
                          dy_tm: bool = False, x_tm: bool = False) -> None:
    _lib.call('ft_linear_bwd_weight', dy_ptr, lddy, x_ptr, ldx, _p(dw), rows, in_f, out_f, B, T if T else rows,
              x_shift, int(accumulate), int(dy_tm), int(x_tm),
              *scratch('ft_linear_bwd_weight_workspace', rows, in_f, out_f, device=dw.device), _stream())


def linear_bwd_weight(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """dw[out,in] = dy^T x over all leading positions."""
    _chk(dy, 'dy'); _chk(x, 'x')
    out_f, in_f = dy.shape[-1], x.shape[-1]
    rows = x.numel() // max(in_f, 1)
    dw = torch.empty(out_f, in_f, device=x.device, dtype=x.dtype)
    linear_bwd_weight_raw(_p(dy), out_f, _p(x), in_f, dw, rows, in_f, out_f)
    return dw


# ---------------------------------------------------------------------------------------------------
# per-step operand packs
# ---------------------------------------------------------------------------------------------------
class PackCache:
    """Every re-laid-out copy of a model's weights the GEMM kernels consume -- tap-major conv packs [k,Cout,Cin],
    their transposes [k,Cin,Cout], the contiguous per-bank concatenations of both, and W^T of every matrix -- kept in
    persistent buffers and refreshed by ONE ft_pack_weights launch.  Weights change only at the optimizer step, so a
    training step calls refresh() once up front instead of ~120 small per-layer launches spread over forward and
    backward.  Only valid between a refresh() and the next weight update: the owner (trainer.TrainStep) installs it as
    `hip.pack_cache` for the duration of one step and removes it afterwards; with no cache installed every wrapper
    below packs on the fly as before.

    mats: 2-D weights; convs: 3-D Conv1d weights used on their own; banks: lists of Conv1d weights (k = 1..K, equal
    [C,Cin]) whose packs must sit back to back (CBHG conv bank)."""

    def __init__(self, mats, convs, banks, device, highways=()):
        """highways: (W1, W2) pairs of HighwayNetworks whose width is a multiple of 32 -> their 32-row interleave
        (ft_highway_pack layout), the B operand of the fused highway forward"""
        import struct
        self.wp, self.wpt, self.t2d, self.bank, self.hw = {}, {}, {}, {}, {}
        self._keep = []
        descs = []
        tiles = 0

        def add(src, dst, dst_t, d0, d1, k):
            nonlocal tiles
            descs.append(struct.pack('PPPqiiii', src.data_ptr(), _p(dst) or 0, _p(dst_t) or 0, tiles, d0, d1, k, 0))
            tiles += k * ((d0 + 31) // 32) * ((d1 + 31) // 32)

        for w in mats:
            _chk(w, 'w')
            R, C = w.shape
            wt = torch.empty(C, R, device=device, dtype=w.dtype)
            self.t2d[(w.data_ptr(), R, C)] = wt
            add(w, None, wt, R, C, 1)
        for w in convs:
            _chk(w, 'w')
            Cout, Cin, k = w.shape
            wp = torch.empty(k, Cout, Cin, device=device, dtype=w.dtype)
            wpt = torch.empty(k, Cin, Cout, device=device, dtype=w.dtype)
            self.wp[w.data_ptr()] = wp
            self.wpt[w.data_ptr()] = wpt
            add(w, wp, wpt, Cout, Cin, k)
        for ws in banks:
            C, Cin = ws[0].shape[0], ws[0].shape[1]
            n = sum(w.shape[2] for w in ws) * C * Cin
            wp_all = torch.empty(n, device=device, dtype=ws[0].dtype)
            wpt_all = torch.empty(n, device=device, dtype=ws[0].dtype)
            off = 0
            for w in ws:
                _chk(w, 'w')
                k = w.shape[2]
                add(w, wp_all[off:off + k * C * Cin], wpt_all[off:off + k * C * Cin], C, Cin, k)
                off += k * C * Cin
            self.bank[tuple(w.data_ptr() for w in ws)] = (wp_all, wpt_all)
        for w1, w2 in highways:
            _chk(w1, 'w1'); _chk(w2, 'w2')
            C = w1.shape[0]
            if w1.shape != (C, C) or w2.shape != (C, C) or C % 32:
                continue
            pack = torch.empty(2 * C, C, device=device, dtype=w1.dtype)
            self.hw[(w1.data_ptr(), w2.data_ptr())] = pack
            for j in range(C // 32):        # plain [32, C] row-block copies (dst only, one tap)
                add(w1[32 * j:32 * j + 32], pack[64 * j:64 * j + 32], None, 32, C, 1)
                add(w2[32 * j:32 * j + 32], pack[64 * j + 32:64 * j + 64], None, 32, C, 1)
        self.n, self.tiles = len(descs), tiles
        self.descs = torch.frombuffer(bytearray(b''.join(descs)), dtype=torch.uint8).to(device) if descs else None

    def refresh(self) -> None:
        if self.n:
            _lib.call('ft_pack_weights', _p(self.descs), self.n, self.tiles, _stream())

    @staticmethod
    def release() -> None:
        """the weights are about to change (or the step failed): the packs are stale until the next refresh()"""


pack_cache: Optional[PackCache] = None


def bank_packs(ws: Sequence[torch.Tensor], transposed: bool) -> torch.Tensor:
    """back-to-back tap-major packs ([k,C,Cin], or [k,Cin,C] if transposed) of the members of a conv bank"""
    if pack_cache is not None:
        hit = pack_cache.bank.get(tuple(w.data_ptr() for w in ws))
        if hit is not None:
            return hit[1 if transposed else 0]
    C, Cin = ws[0].shape[0], ws[0].shape[1]
    out = torch.empty(sum(w.shape[2] for w in ws) * C * Cin, device=ws[0].device, dtype=ws[0].dtype)
    off = 0
    for w in ws:
        k = w.shape[2]
        n = k * C * Cin
        if transposed:
            conv_pack_weight_t(w, out=out[off:off + n].view(k, Cin, C))
        else:
            conv_pack_weight(w, out=out[off:off + n].view(k, C, Cin))
        off += n
    return out


# ---------------------------------------------------------------------------------------------------
# channels-last conv
# ---------------------------------------------------------------------------------------------------
def conv_pack_weight(w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[Cout,Cin,k] -> tap-major [k,Cout,Cin]"""
    if out is None and pack_cache is not None:
        hit = pack_cache.wp.get(w.data_ptr())
        if hit is not None:
            return hit
    _chk(w, 'w')
    Cout, Cin, k = w.shape
    wp = out if out is not None else torch.empty(k, Cout, Cin, device=w.device, dtype=w.dtype)
    _lib.call('ft_conv_pack_weight', _p(w), _p(wp), Cout, Cin, k, _stream())
    return wp


def conv1d_fwd(x: torch.Tensor, wp: torch.Tensor, relu: bool, Tout: Optional[int] = None,
               scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
               accumulate_into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B,T,Cin], wp [k,Cout,Cin] -> y [B,Tout,Cout]; accumulate_into: result is ADDED onto that tensor"""
    _chk(x, 'x'); _chk(wp, 'wp')
    B, T, Cin = x.shape
    k, Cout, _ = wp.shape
    Tout = T if Tout is None else Tout
    y = accumulate_into if accumulate_into is not None else torch.empty(B, Tout, Cout, device=x.device,
                                                                        dtype=x.dtype)
    _lib.call('ft_conv1d_fwd', _p(x), Cin, _p(wp), _p(scale), _p(shift), _p(y), Cout, B, T, Cin, Cout, k, Tout,
              int(relu), int(accumulate_into is not None), _stream())
    return y


def conv1d_fwd_lens(x: torch.Tensor, wp: torch.Tensor, relu: bool, lens: torch.Tensor,
                    scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
                    accumulate_into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv1d_fwd at Tout = T whose epilogue stores zeros at t >= lens[b] (lens int64 [B], device)"""
    _chk(x, 'x'); _chk(wp, 'wp'); _chk(lens, 'lens', torch.int64)
    B, T, Cin = x.shape
    k, Cout, _ = wp.shape
    assert lens.numel() == B
    y = accumulate_into if accumulate_into is not None else torch.empty(B, T, Cout, device=x.device, dtype=x.dtype)
    _lib.call('ft_conv1d_fwd_lens', _p(x), Cin, _p(wp), _p(scale), _p(shift), _p(y), Cout, _p(lens), B, T, Cin, Cout, k,
              int(relu), int(accumulate_into is not None), _stream())
    return y


def conv1d_bias_fwd_lens(x: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, relu: bool, lens: torch.Tensor) -> torch.Tensor:
    """nn.Conv1d with bias (+ ReLU) on a ragged batch: x [B,T,Cin] (zero at t >= lens[b]), wp [k,Cout,Cin], k odd ->
    y [B,T,Cout], exactly +0.0 at t >= lens[b] (stored, not multiplied: neither the bias nor a NaN survives there).  The
    rows lens[b] <= t < lens[b] + k//2 of x are read into valid rows and must be zero; rows at t >= lens[b] + k//2 are
    never read into a valid row and may hold anything.  A length above T counts as T."""
    _chk(x, 'x'); _chk(wp, 'wp'); _chk(bias, 'bias'); _chk(lens, 'lens', torch.int64)
    B, T, Cin = x.shape
    k, Cout, _ = wp.shape
    assert lens.numel() == B
    y = torch.empty(B, T, Cout, device=x.device, dtype=x.dtype)
    _lib.call('ft_conv1d_bias_fwd_lens', _p(x), Cin, _p(wp), _p(bias), _p(y), Cout, _p(lens), B, T, Cin, Cout, k,
              int(relu), _stream())
    return y


def add_layernorm_fwd_lens(x: torch.Tensor, res: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                           lens: torch.Tensor, eps: float) -> torch.Tensor:
    """LayerNorm(x + res) (res may be None) of a ragged batch [B,T,D]: exactly 0 at t >= lens[b], where neither input
    is read.  Inference only: nothing is saved for a backward."""
    _chk(x, 'x'); _chk(lens, 'lens', torch.int64)
    if res is not None:
        _chk(res, 'res')
    B, T, D = x.shape
    assert lens.numel() == B
    y = torch.empty_like(x)
    _lib.call('ft_add_layernorm_fwd_lens', _p(x), _p(res), _p(gamma), _p(beta), _p(lens), _p(y), B, T, D, float(eps),
              _stream())
    return y


def conv_bank_fwd(x: torch.Tensor, wp_all: torch.Tensor, K: int, C: int, relu: bool, Tout: int,
                  scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B,T,Cin]; wp_all flat packed weights of members k=1..K -> ybank [B,Tout,K*C]"""
    _chk(x, 'x'); _chk(wp_all, 'wp_all')
    B, T, Cin = x.shape
    assert wp_all.numel() == C * Cin * K * (K + 1) // 2
    y = torch.empty(B, Tout, K * C, device=x.device, dtype=x.dtype)
    _lib.call('ft_conv_bank_fwd', _p(x), Cin, _p(wp_all), _p(scale), _p(shift), _p(y), B, T, Cin, C, K, Tout,
              int(relu), _stream())
    return y


def conv1d_fwd_stats(x: torch.Tensor, wp: torch.Tensor, relu: bool, Tout: int):
    """conv (+ReLU) whose GEMM epilogue also leaves the BatchNorm statistics partials of y behind
    (include/fwdtaco_hip.h: ft_conv1d_fwd_stats).  -> (y [B,Tout,Cout], partial buffer, nchunks)"""
    _chk(x, 'x'); _chk(wp, 'wp')
    B, T, Cin = x.shape
    k, Cout, _ = wp.shape
    y = torch.empty(B, Tout, Cout, device=x.device, dtype=x.dtype)
    nbytes = _lib.query('ft_conv1d_fwd_stats_workspace', B, Tout, Cout, k)
    part = workspace(nbytes, x.device)
    n = ctypes.c_int(0)
    _lib.call('ft_conv1d_fwd_stats', _p(x), Cin, _p(wp), _p(y), Cout, B, T, Cin, Cout, k, Tout, int(relu), _p(part),
              part.numel(), ctypes.byref(n), _stream())
    return y, part, n.value


def conv_bank_fwd_stats(x: torch.Tensor, wp_all: torch.Tensor, K: int, C: int, relu: bool):
    """training-mode conv bank: ybank [B,T+1,K*C] + the statistics partials of its K BatchNorms"""
    _chk(x, 'x'); _chk(wp_all, 'wp_all')
    B, T, Cin = x.shape
    assert wp_all.numel() == C * Cin * K * (K + 1) // 2
    y = torch.empty(B, T + 1, K * C, device=x.device, dtype=x.dtype)
    nbytes = _lib.query('ft_conv_stats_workspace', B, T + 1, K * C)
    part = workspace(nbytes, x.device)
    n = ctypes.c_int(0)
    _lib.call('ft_conv_bank_fwd_stats', _p(x), Cin, _p(wp_all), _p(y), B, T, Cin, C, K, int(relu), _p(part),
              part.numel(), ctypes.byref(n), _stream())
    return y, part, n.value


def bn_train_from_partials(part: torch.Tensor, nchunks: int, y: torch.Tensor, gamma, beta, running_mean, running_var,
                           Tout: int, group: int = 0, residual: Optional[torch.Tensor] = None,
                           momentum: float = None, eps: float = None):
    """finalize the statistics partials (ordered) + normalise: -> (out [B,Tout,C], save_mean, save_rstd)"""
    B, Tbuf, C = y.shape
    out = torch.empty(B, Tout, C, device=y.device, dtype=y.dtype)
    mean = torch.empty(C, device=y.device, dtype=y.dtype)
    rstd = torch.empty(C, device=y.device, dtype=y.dtype)
    _lib.call('ft_bn_train_from_partials', _p(part), nchunks, _p(y), _p(gamma), _p(beta), _p(residual), _p(out),
              _p(running_mean), _p(running_var), None, _p(mean), _p(rstd), B, Tbuf, Tout, C, group,
              BN_MOMENTUM if momentum is None else momentum, BN_EPS if eps is None else eps, _stream())
    return out, mean, rstd


def conv_pack_weight_t(w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[Cout,Cin,k] -> transposed tap-major [k,Cin,Cout] (weight operand of the data gradient in the NT form)"""
    if out is None and pack_cache is not None:
        hit = pack_cache.wpt.get(w.data_ptr())
        if hit is not None:
            return hit
    _chk(w, 'w')
    Cout, Cin, k = w.shape
    wpt = out if out is not None else torch.empty(k, Cin, Cout, device=w.device, dtype=w.dtype)
    _lib.call('ft_conv_pack_weight_t', _p(w), _p(wpt), Cout, Cin, k, _stream())
    return wpt


def conv1d_bwd_data_raw(dy_ptr: int, lddy: int, wp: torch.Tensor, dx: torch.Tensor, B: int, T: int, Tbuf: int,
                        Tvalid: int, accumulate: bool, w: Optional[torch.Tensor] = None) -> None:
    """wp: packed [k,Cout,Cin]; with the original weight `w` at hand (and Cout % 4 == 0) the NT form is used"""
    k, Cout, Cin = wp.shape
    if NT_GRADS and w is not None and Cout % 4 == 0:
        wpt = conv_pack_weight_t(w)
        _lib.call('ft_conv1d_bwd_data', dy_ptr, lddy, _p(wpt), _p(dx), Cin, B, T, Cin, Cout, k, Tbuf, Tvalid,
                  int(accumulate), 1, _stream())
        return
    _lib.call('ft_conv1d_bwd_data', dy_ptr, lddy, _p(wp), _p(dx), Cin, B, T, Cin, Cout, k, Tbuf, Tvalid,
              int(accumulate), 0, _stream())


def conv1d_bwd_data_relu(dy: torch.Tensor, w: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The data gradient of nn.Conv1d(Cin, Cout, k, padding=k//2) through the ReLU in front of it, in ONE launch:
    dy [B,T,Cout], w [Cout,Cin,k], y [B,T,Cin] = the OUTPUT of the conv + ReLU this convolution read -> dx [B,T,Cin] =
    (dy * w) where y > 0, exactly 0 elsewhere (include/fwdtaco_hip.h: ft_conv1d_bwd_data_relu).  The weight operand goes in
    the form conv1d_bwd_data_raw picks for the same w."""
    _chk(dy, 'dy'); _chk(w, 'w'); _chk(y, 'y')
    B, T, Cout = dy.shape
    Cin, k = w.shape[1], w.shape[2]
    if w.shape[0] != Cout or tuple(y.shape) != (B, T, Cin):
        raise _lib.FtError(f'conv1d_bwd_data_relu: dy {tuple(dy.shape)}, w {tuple(w.shape)}, y {tuple(y.shape)} do not match')
    flag = int(NT_GRADS and Cout % 4 == 0)
    wp = conv_pack_weight_t(w) if flag else conv_pack_weight(w)
    dx = torch.empty(B, T, Cin, device=dy.device, dtype=dy.dtype)
    _lib.call('ft_conv1d_bwd_data_relu', _p(dy), Cout, _p(wp), _p(y), _p(dx), Cin, B, T, Cin, Cout, k, flag, _stream())
    return dx


def conv_bank_bwd_data(dy: torch.Tensor, wp_all: torch.Tensor, K: int, C: int, Cin: int, T: int,
                       ws: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
    """dy [B,Tbuf,K*C] (gradient of the bank buffer) -> dx [B,T,Cin], all K members in one chained launch.
    ws: the members' original [C,Cin,k] weights -> transposed packs, NT form."""
    _chk(dy, 'dy'); _chk(wp_all, 'wp_all')
    B, Tbuf, _ = dy.shape
    dx = torch.empty(B, T, Cin, device=dy.device, dtype=dy.dtype)
    flag = 0
    if NT_GRADS and ws is not None and C % 4 == 0:
        wp_all, flag = bank_packs(ws, True), 1
    nbytes = _lib.query('ft_conv_bank_bwd_data_workspace', B, T, Cin, K)
    ws = workspace(nbytes, dy.device) if nbytes else None
    _lib.call('ft_conv_bank_bwd_data', _p(dy), K * C, _p(wp_all), _p(dx), Cin, B, T, Cin, C, K, Tbuf, flag,
              _p(ws), ws.numel() if ws is not None else 0, _stream())
    return dx


def conv_bank_bwd_weight(dy: torch.Tensor, x: torch.Tensor, dws: Sequence[torch.Tensor], C: int) -> None:
    """dy [B,Tbuf,K*C] gradient of the bank buffer, x [B,T,Cin]; overwrites dws[i] ([C,Cin,i+1]) for all K members
    with one GEMM launch (C % 128 == 0)."""
    _chk(dy, 'dy'); _chk(x, 'x')
    B, T, Cin = x.shape
    Tbuf, K = dy.shape[1], len(dws)
    for i, d in enumerate(dws):
        _chk(d, 'dw')
        if tuple(d.shape) != (C, Cin, i + 1):
            raise _lib.FtError(f'conv_bank_bwd_weight: dw[{i}] has shape {tuple(d.shape)}')
    _lib.call('ft_conv_bank_bwd_weight', _p(dy), K * C, _p(x), Cin, _ptr_array(dws), B, T, Cin, C, K, Tbuf,
              *scratch('ft_conv_bank_bwd_weight_workspace', B, T, Cin, C, K, Tbuf, device=x.device), _stream())


def conv1d_bwd_weight_raw(dy_ptr: int, lddy: int, x: torch.Tensor, dw: torch.Tensor, Tbuf: int, Tvalid: int) -> None:
    B, T, Cin = x.shape
    Cout, _, k = dw.shape
    _lib.call('ft_conv1d_bwd_weight', dy_ptr, lddy, _p(x), Cin, _p(dw), B, T, Cin, Cout, k, Tbuf, Tvalid,
              *scratch('ft_conv1d_bwd_weight_workspace', B, T, Cin, Cout, k, Tvalid, device=x.device), _stream())


# ---------------------------------------------------------------------------------------------------
# LengthRegulator
# ---------------------------------------------------------------------------------------------------
def lr_scan(dur: torch.Tensor):
    """In-place clamp of dur (<0 -> 0) + prefix sums.  Returns (cum int32 [B,Tx+1], total int32 [B])."""
    _chk(dur, 'dur')
    B, Tx = dur.shape
    cum = torch.empty(B, Tx + 1, device=dur.device, dtype=torch.int32)
    total = torch.empty(B, device=dur.device, dtype=torch.int32)
    _lib.call('ft_lr_scan', _p(dur), B, Tx, _p(cum), _p(total), _stream())
    return cum, total


def gen_durations(dur: torch.Tensor, x_len: torch.Tensor):
    """Per-item duration fallback, mask and clamp of a ragged inference batch, in place on dur [B,Tx] (ft_gen_durations).
    -> (mel_len int64 [B], bad int32 [1]: non-zero if an x_len was outside [1, Tx])"""
    _chk(dur, 'dur'); _chk(x_len, 'x_len', torch.int64)
    B, Tx = dur.shape
    assert x_len.numel() == B
    mel_len = torch.empty(B, device=dur.device, dtype=torch.int64)
    bad = torch.zeros(1, device=dur.device, dtype=torch.int32)
    _lib.call('ft_gen_durations', _p(dur), _p(x_len), B, Tx, _p(mel_len), _p(bad), _stream())
    return mel_len, bad


def lr_expand(x: torch.Tensor, cum: torch.Tensor, Tm: int, want_src: bool = False):
    _chk(x, 'x'); _chk(cum, 'cum', torch.int32)
    B, Tx, C = x.shape
    y = torch.empty(B, Tm, C, device=x.device, dtype=x.dtype)
    src = torch.empty(B, Tm, device=x.device, dtype=torch.int32) if want_src else None
    _lib.call('ft_lr_expand', _p(x), _p(cum), _p(y), _p(src), B, Tx, Tm, C, _stream())
    return (y, src) if want_src else y


def lr_bwd(dy: torch.Tensor, cum: torch.Tensor, Tx: int) -> torch.Tensor:
    _chk(dy, 'dy'); _chk(cum, 'cum', torch.int32)
    B, Tm, C = dy.shape
    dx = torch.empty(B, Tx, C, device=dy.device, dtype=dy.dtype)
    _lib.call('ft_lr_bwd', _p(dy), _p(cum), _p(dx), B, Tx, Tm, C, _stream())
    return dx


def lr_expand_tm(x: torch.Tensor, cum: torch.Tensor, Tm: int, pad_row: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B,Tx,C] -> TIME-major [Tm,B,C]; frames beyond an item's length hold pad_row (zeros if None)"""
    _chk(x, 'x'); _chk(cum, 'cum', torch.int32)
    B, Tx, C = x.shape
    if pad_row is not None:
        _chk(pad_row, 'pad_row')
        assert pad_row.numel() == C
    y = torch.empty(Tm, B, C, device=x.device, dtype=x.dtype)
    _lib.call('ft_lr_expand_tm', _p(x), _p(cum), _p(pad_row), _p(y), B, Tx, Tm, C, _stream())
    return y


def lr_bwd_tm(dy: torch.Tensor, cum: torch.Tensor, Tx: int):
    """dy TIME-major [Tm,B,C] -> (dx [B,Tx,C]: the frames of every token added up, in frame order; rows [B*Tx + B, C]:
    dx's rows followed by one row per item with the sum of the frames beyond its last token -- what a column sum over
    ALL frames has to run over)"""
    _chk(dy, 'dy'); _chk(cum, 'cum', torch.int32)
    Tm, B, C = dy.shape
    rows = torch.empty(B * Tx + B, C, device=dy.device, dtype=dy.dtype)
    dx = rows[:B * Tx].view(B, Tx, C)
    _lib.call('ft_lr_bwd_tm', _p(dy), _p(cum), _p(dx), _p(rows[B * Tx:]), B, Tx, Tm, C, _stream())
    return dx, rows


# ---------------------------------------------------------------------------------------------------
# BatchNorm / column sums
# ---------------------------------------------------------------------------------------------------
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def bn_train_fwd(y: torch.Tensor, gamma, beta, running_mean, running_var, Tout: int, group: int = 0,
                 residual: Optional[torch.Tensor] = None, momentum: float = BN_MOMENTUM, eps: float = BN_EPS):
    """y [B,Tbuf,C] -> (out [B,Tout,C], save_mean, save_rstd); running stats updated in place."""
    _chk(y, 'y')
    B, Tbuf, C = y.shape
    out = torch.empty(B, Tout, C, device=y.device, dtype=y.dtype)
    mean = torch.empty(C, device=y.device, dtype=y.dtype)
    rstd = torch.empty(C, device=y.device, dtype=y.dtype)
    _lib.call('ft_bn_train_fwd', _p(y), _p(gamma), _p(beta), _p(residual), _p(out), _p(running_mean),
              _p(running_var), None, _p(mean), _p(rstd), B, Tbuf, Tout, C, group, momentum, eps,
              *scratch('ft_bn_workspace', B, Tbuf, C, device=y.device), _stream())
    return out, mean, rstd


def bn_bwd(dout: torch.Tensor, y: torch.Tensor, gamma, mean, rstd, group: int, relu: bool,
           dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None):
    """-> (dy [B,Tbuf,C], dgamma [C], dbeta [C]); dgamma / dbeta may be caller-provided output buffers"""
    _chk(dout, 'dout'); _chk(y, 'y')
    B, Tbuf, C = y.shape
    Tout = dout.shape[1]
    dy = torch.empty_like(y)
    if dgamma is None:
        dgamma = torch.empty(C, device=y.device, dtype=y.dtype)
    if dbeta is None:
        dbeta = torch.empty(C, device=y.device, dtype=y.dtype)
    _lib.call('ft_bn_bwd', _p(dout), _p(y), _p(gamma), _p(mean), _p(rstd), _p(dy), _p(dgamma), _p(dbeta), B, Tbuf,
              Tout, C, group, int(relu), *scratch('ft_bn_workspace', B, Tbuf, C, device=y.device), _stream())
    return dy, dgamma, dbeta


def bn_pool_fusable(y: torch.Tensor, group: int) -> bool:
    """the fused BatchNorm + MaxPool kernels take the 16-byte path only"""
    return y.shape[-1] % 4 == 0 and group % 4 == 0 and y.data_ptr() % 16 == 0


def bn_pool_from_partials(part: torch.Tensor, nchunks: int, y: torch.Tensor, gamma, beta, running_mean, running_var,
                          Tout: int, group: int = 0, momentum: float = None, eps: float = None):
    """finalize the statistics partials + MaxPool1d(2,1,1)(bn(y))[:Tout] in one pass over y (the normalised tensor is
    never stored): -> (out [B,Tout,C], save_mean, save_rstd)"""
    B, Tbuf, C = y.shape
    out = torch.empty(B, Tout, C, device=y.device, dtype=y.dtype)
    mean = torch.empty(C, device=y.device, dtype=y.dtype)
    rstd = torch.empty(C, device=y.device, dtype=y.dtype)
    _lib.call('ft_bn_pool_from_partials', _p(part), nchunks, _p(y), _p(gamma), _p(beta), _p(out), _p(running_mean),
              _p(running_var), None, _p(mean), _p(rstd), B, Tbuf, Tout, C, group,
              BN_MOMENTUM if momentum is None else momentum, BN_EPS if eps is None else eps, _stream())
    return out, mean, rstd


def bn_pool_bwd(dout: torch.Tensor, y: torch.Tensor, gamma, beta, mean, rstd, group: int, relu: bool):
    """backward of bn_pool_from_partials: dout = gradient of the pooled output -> (dy [B,Tbuf,C], dgamma, dbeta)"""
    _chk(dout, 'dout'); _chk(y, 'y')
    B, Tbuf, C = y.shape
    Tout = dout.shape[1]
    dy = torch.empty_like(y)
    dgamma = torch.empty(C, device=y.device, dtype=y.dtype)
    dbeta = torch.empty(C, device=y.device, dtype=y.dtype)
    _lib.call('ft_bn_pool_bwd', _p(dout), _p(y), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dy), _p(dgamma), _p(dbeta),
              B, Tbuf, Tout, C, group, int(relu), *scratch('ft_bn_workspace', B, Tbuf, C, device=y.device), _stream())
    return dy, dgamma, dbeta


def bn_fold_eval(gamma, beta, running_mean, running_var, eps: float = BN_EPS):
    C = gamma.numel()
    scale = torch.empty(C, device=gamma.device, dtype=gamma.dtype)
    shift = torch.empty(C, device=gamma.device, dtype=gamma.dtype)
    _lib.call('ft_bn_fold_eval', _p(gamma), _p(beta), _p(running_mean), _p(running_var), eps, _p(scale), _p(shift),
              C, _stream())
    return scale, shift


def colsum_raw(x_ptr: int, ldx: int, out: torch.Tensor, rows: int, C: int, scale: float = 1.0,
               accumulate: bool = False) -> None:
    _lib.call('ft_colsum', x_ptr, ldx, _p(out), rows, C, scale, int(accumulate),
              *scratch('ft_colsum_workspace', rows, C, device=out.device), _stream())


def colsum2_raw(x0_ptr: int, x1_ptr: int, ldx: int, out0: torch.Tensor, out1: torch.Tensor, rows: int, C: int) -> None:
    """out0 = column sums of x0, out1 = of x1 (same [rows, C] shape, row stride ldx): one partial + one finalize launch"""
    _lib.call('ft_colsum2', x0_ptr, x1_ptr, ldx, _p(out0), _p(out1), rows, C,
              *scratch('ft_colsum_workspace', rows, C, device=out0.device), _stream())


def colsum(x: torch.Tensor) -> torch.Tensor:
    _chk(x, 'x')
    C = x.shape[-1]
    rows = x.numel() // max(C, 1)
    out = torch.empty(C, device=x.device, dtype=x.dtype)
    colsum_raw(_p(x), C, out, rows, C)
    return out


def colsum_batch(xs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """column sums of up to 16 matrices with the same row count in one partial + one finalize launch (each bit-identical
    to colsum of that matrix)"""
    rows = xs[0].numel() // xs[0].shape[-1]
    for x in xs:
        _chk(x, 'x')
        assert x.numel() // x.shape[-1] == rows
    n = len(xs)
    outs = [torch.empty(x.shape[-1], device=x.device, dtype=x.dtype) for x in xs]
    Cs = (ctypes.c_int * n)(*[int(x.shape[-1]) for x in xs])
    lds = (ctypes.c_long * n)(*[int(x.shape[-1]) for x in xs])
    nbytes = _lib.lib().ft_colsum_batch_workspace(n, ctypes.cast(Cs, c_void_p), rows)
    ws = workspace(max(int(nbytes), 16), xs[0].device)
    _lib.call('ft_colsum_batch', n, ctypes.cast(_ptr_array(list(xs)), c_void_p), ctypes.cast(lds, c_void_p),
              ctypes.cast(_ptr_array(outs), c_void_p), ctypes.cast(Cs, c_void_p), rows, _p(ws), ws.numel(), _stream())
    return outs


# ---------------------------------------------------------------------------------------------------
# element-wise
# ---------------------------------------------------------------------------------------------------
def dropout(x: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    _chk(x, 'x')
    out = torch.empty_like(x)
    _lib.call('ft_dropout', _p(x), _p(out), x.numel(), p, seed & 0xFFFFFFFFFFFFFFFF, _stream())
    return out


def scale(x: torch.Tensor, s: float) -> torch.Tensor:
    _chk(x, 'x')
    out = torch.empty_like(x)
    _lib.call('ft_scale', _p(x), _p(out), x.numel(), s, _stream())
    return out



def embedding_fwd(idx: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    _chk(idx, 'idx', torch.int64); _chk(w, 'w')
    V, C = w.shape
    out = torch.empty(*idx.shape, C, device=w.device, dtype=w.dtype)
    err = _err_flag(w.device)
    _lib.call('ft_embedding_fwd', _p(idx), _p(w), _p(out), idx.numel(), C, V, _p(err), _stream())
    return out


def embedding_fwd_lens(idx: torch.Tensor, lens: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """idx [B,T], lens int64 [B] (device) -> [B,T,C]: embedding_fwd with zeros at t >= lens[b], where idx is not read"""
    _chk(idx, 'idx', torch.int64); _chk(lens, 'lens', torch.int64); _chk(w, 'w')
    B, T = idx.shape
    assert lens.numel() == B
    V, C = w.shape
    out = torch.empty(B, T, C, device=w.device, dtype=w.dtype)
    _lib.call('ft_embedding_fwd_lens', _p(idx), _p(lens), _p(w), _p(out), B, T, C, V, _p(_err_flag(w.device)), _stream())
    return out


def predictor_front_lens(idx: torch.Tensor, lens: torch.Tensor, w: torch.Tensor, cond: Optional[torch.Tensor] = None,
                         cond_w: Optional[torch.Tensor] = None, semb: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The front of a speaker-conditioned predictor on a ragged batch: idx [B,T] (and cond [B,T]) int64, lens int64 [B]
    (device), semb [B,S] one row per item -> [B,T,Ce+Cc+S] = [ w[idx] | cond_w[cond] | semb[b] ] at t < lens[b], zeros at
    t >= lens[b], where idx / cond are not read.  cond (with cond_w) and semb are optional."""
    _chk(idx, 'idx', torch.int64); _chk(lens, 'lens', torch.int64); _chk(w, 'w')
    B, T = idx.shape
    assert lens.numel() == B
    V, Ce = w.shape
    Vc = Cc = S = 0
    if cond is not None:
        _chk(cond, 'cond', torch.int64); _chk(cond_w, 'cond_w')
        assert cond.shape == idx.shape
        Vc, Cc = cond_w.shape
    if semb is not None:
        _chk(semb, 'semb')
        assert semb.dim() == 2 and semb.shape[0] == B
        S = semb.shape[1]
    out = torch.empty(B, T, Ce + Cc + S, device=w.device, dtype=w.dtype)
    _lib.call('ft_predictor_front_lens', _p(idx), _p(cond), _p(lens), _p(w), Ce, V, _p(cond_w) if cond is not None else None,
              Cc, Vc, _p(semb), S, _p(out), B, T, _p(_err_flag(w.device)), _stream())
    return out


def argmax_lens(logits: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """logits [B,T,K], lens int64 [B] (device) -> int64 [B,T]: torch.argmax over K at t < lens[b], 0 at t >= lens[b]"""
    _chk(logits, 'logits'); _chk(lens, 'lens', torch.int64)
    B, T, K = logits.shape
    assert lens.numel() == B
    out = torch.empty(B, T, device=logits.device, dtype=torch.int64)
    _lib.call('ft_argmax_lens', _p(logits), _p(lens), _p(out), B, T, K, _stream())
    return out


def check_tokens_lens(idx: torch.Tensor, lens: torch.Tensor, flag: torch.Tensor) -> None:
    """flag[0] |= 2 (int32, device) if idx [B,T] holds the pad id 0 at some t < lens[b]"""
    _chk(idx, 'idx', torch.int64); _chk(lens, 'lens', torch.int64); _chk(flag, 'flag', torch.int32)
    B, T = idx.shape
    assert lens.numel() == B
    _lib.call('ft_check_tokens_lens', _p(idx), _p(lens), B, T, _p(flag), _stream())


_err_flags = {}


def _err_flag(device) -> torch.Tensor:
    key = torch.device(device).index or 0
    if key not in _err_flags:
        _err_flags[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _err_flags[key]


def check_index_errors(device) -> None:
    """Host-side check of the out-of-range embedding index flag (syncs)."""
    f = _err_flag(device)
    if int(f.item()) != 0:
        f.zero_()
        raise IndexError('embedding index out of range (set by ft_embedding_fwd)')


def onehot(idx: torch.Tensor, V: int) -> torch.Tensor:
    _chk(idx, 'idx', torch.int64)
    out = torch.empty(idx.numel(), V, device=idx.device, dtype=torch.float32)
    _lib.call('ft_onehot', _p(idx), _p(out), idx.numel(), V, _stream())
    return out


def embedding_bwd(idx: torch.Tensor, dout: torch.Tensor, V: int,
                  onehot_cache: Optional[dict] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW[V,C] = onehot(idx)^T @ dout (TN MFMA GEMM).  onehot_cache lets the four embedding tables that
    share one id tensor (main + three predictors) build the one-hot matrix once."""
    _chk(idx, 'idx', torch.int64); _chk(dout, 'dout')
    C = dout.shape[-1]
    key = (idx.data_ptr(), idx.numel(), V, _stream())          # per stream: no cross-stream sharing
    oh = onehot_cache.get(key) if onehot_cache is not None else None
    if oh is None:
        oh = onehot(idx, V)
        if onehot_cache is not None:
            onehot_cache[key] = oh
    dw = out if out is not None else torch.empty(V, C, device=dout.device, dtype=dout.dtype)
    linear_bwd_weight_raw(_p(oh), V, _p(dout), C, dw, idx.numel(), C, V)
    return dw


def highway_gate_fwd(x12: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    _chk(x12, 'x12'); _chk(x, 'x')
    C = x.shape[-1]
    out = torch.empty_like(x)
    _lib.call('ft_highway_gate_fwd', _p(x12), _p(x), _p(out), x.numel() // C, C, _stream())
    return out


def highway_gate_bwd(dout, x12, x):
    _chk(dout, 'dout')
    C = x.shape[-1]
    d12 = torch.empty_like(x12)
    dx = torch.empty_like(x)
    _lib.call('ft_highway_gate_bwd', _p(dout), _p(x12), _p(x), _p(d12), _p(dx), x.numel() // C, C, _stream())
    return d12, dx


def highway_pack(w1: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """the 32-row interleave [2C, C] of W1 / W2 (include/fwdtaco_hip.h: ft_highway_pack); from the step's PackCache if it
    holds this pair"""
    if pack_cache is not None:
        hit = pack_cache.hw.get((w1.data_ptr(), w2.data_ptr()))
        if hit is not None:
            return hit
    _chk(w1, 'w1'); _chk(w2, 'w2')
    C = w1.shape[0]
    out = torch.empty(2 * C, C, device=w1.device, dtype=w1.dtype)
    _lib.call('ft_highway_pack', _p(w1), _p(w2), _p(out), C, _stream())
    return out


def highway_fwd(x: torch.Tensor, w12i: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor, save: bool):
    """HighwayNetwork forward with the gate in the GEMM epilogue -> (out [.., C], x12 [.., 2C] or None)"""
    _chk(x, 'x'); _chk(w12i, 'w12i')
    C = x.shape[-1]
    rows = x.numel() // C
    out = torch.empty_like(x)
    x12 = torch.empty(*x.shape[:-1], 2 * C, device=x.device, dtype=x.dtype) if save else None
    _lib.call('ft_highway_fwd', _p(x), _p(w12i), _p(b1), _p(b2), _p(out), _p(x12), rows, C, _stream())
    return out, x12


def highway_bwd_data(d12: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, dx: torch.Tensor,
                     below: Optional[tuple] = None) -> Optional[torch.Tensor]:
    """dx += d12[:, :C] W1 + d12[:, C:] W2 (in place; dx holds the direct-path term).  below = (x12, x) of the highway
    layer underneath: dx then becomes THAT layer's direct-path term and its gate gradients d12 [.., 2C] are returned."""
    C = dx.shape[-1]
    rows = dx.numel() // C
    flag = 1 if NT_GRADS else 0
    wa, wb = (transpose2d(w1), transpose2d(w2)) if flag else (w1, w2)
    d12b = torch.empty_like(d12) if below is not None else None
    _lib.call('ft_highway_bwd_data', _p(d12), _p(wa), _p(wb), flag, _p(dx), rows, C,
              _p(below[0]) if below else None, _p(below[1]) if below else None, _p(d12b), _stream())
    return d12b


def maxpool2_fwd(x: torch.Tensor) -> torch.Tensor:
    _chk(x, 'x')
    B, T, C = x.shape
    out = torch.empty_like(x)
    _lib.call('ft_maxpool2_fwd', _p(x), _p(out), B, T, C, _stream())
    return out


def maxpool2_fwd_lens(x: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """maxpool2_fwd with zeros at t >= lens[b]"""
    _chk(x, 'x'); _chk(lens, 'lens', torch.int64)
    B, T, C = x.shape
    assert lens.numel() == B
    out = torch.empty_like(x)
    _lib.call('ft_maxpool2_fwd_lens', _p(x), _p(lens), _p(out), B, T, C, _stream())
    return out


def maxpool2_bwd(dout: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    _chk(dout, 'dout')
    B, T, C = x.shape
    dx = torch.empty_like(x)
    _lib.call('ft_maxpool2_bwd', _p(dout), _p(x), _p(dx), B, T, C, _stream())
    return dx


def cond_add_fwd(x, pitch, energy, wp, bp, we, be, sp: float, se: float, x_time_major: bool = False) -> torch.Tensor:
    """x [B,T,C] (or time-major [T,B,C]) -> batch-major [B,T,C]"""
    _chk(x, 'x'); _chk(pitch, 'pitch'); _chk(energy, 'energy')
    B, T = pitch.shape
    C = x.shape[-1]
    out = torch.empty(B, T, C, device=x.device, dtype=x.dtype)
    _lib.call('ft_cond_add_fwd', _p(x), _p(pitch), _p(energy), _p(wp), _p(bp), _p(we), _p(be), sp, se, _p(out), B,
              T, C, int(x_time_major), _stream())
    return out


def cond_taps(pitch, energy) -> torch.Tensor:
    B, T = pitch.shape
    taps = torch.empty(B, T, 8, device=pitch.device, dtype=pitch.dtype)
    _lib.call('ft_cond_taps', _p(pitch), _p(energy), _p(taps), B, T, _stream())
    return taps


def concat_cols(a: torch.Tensor, b2: Optional[torch.Tensor], semb: Optional[torch.Tensor], B: int, T: int,
                a_time_major: bool = False) -> torch.Tensor:
    """[a | b2 | broadcast(semb)] along the feature dim -> batch-major [B,T,Ca+Cb+S]"""
    _chk(a, 'a')
    Ca = a.shape[-1]
    Cb = b2.shape[-1] if b2 is not None else 0
    S = semb.shape[-1] if semb is not None else 0
    out = torch.empty(B, T, Ca + Cb + S, device=a.device, dtype=a.dtype)
    _lib.call('ft_concat_cols', _p(a), Ca, _p(b2), Cb, _p(semb), S, _p(out), B, T, int(a_time_major), _stream())
    return out


def slice_cols(src: torch.Tensor, col0: int, C: int, dst_time_major: bool = False) -> torch.Tensor:
    """src batch-major [B,T,ld] -> src[..., col0:col0+C] as a contiguous [B,T,C] (or time-major [T,B,C])"""
    _chk(src, 'src')
    B, T, ld = src.shape
    dst = torch.empty((T, B, C) if dst_time_major else (B, T, C), device=src.device, dtype=src.dtype)
    _lib.call('ft_slice_cols', _p(src), ld, col0, C, _p(dst), B, T, int(dst_time_major), _stream())
    return dst


def cross_entropy_fwd(logits: torch.Tensor, target: torch.Tensor, ignore_index: int):
    _chk(logits, 'logits'); _chk(target, 'target', torch.int64)
    K = logits.shape[-1]
    rows = logits.numel() // K
    loss = torch.empty((), device=logits.device, dtype=logits.dtype)
    inv = torch.empty(1, device=logits.device, dtype=logits.dtype)
    _lib.call('ft_cross_entropy_fwd', _p(logits), _p(target), rows, K, ignore_index, _p(loss), _p(inv),
              *scratch('ft_cross_entropy_workspace', device=logits.device), _stream())
    return loss, inv


def cross_entropy_bwd(logits, target, inv, grad_out, ignore_index: int) -> torch.Tensor:
    K = logits.shape[-1]
    rows = logits.numel() // K
    d = torch.empty_like(logits)
    _lib.call('ft_cross_entropy_bwd', _p(logits), _p(target), _p(inv), _p(grad_out), _p(d), rows, K, ignore_index,
              _stream())
    return d


def transpose_pad_fwd(x: torch.Tensor, Tout: int, pad: float) -> torch.Tensor:
    _chk(x, 'x')
    B, T, C = x.shape
    out = torch.empty(B, C, Tout, device=x.device, dtype=x.dtype)
    _lib.call('ft_transpose_pad_fwd', _p(x), _p(out), B, T, C, Tout, pad, _stream())
    return out


def transpose_pad_lens_fwd(x: torch.Tensor, lens: torch.Tensor, Tout: int, pad: float) -> torch.Tensor:
    """[B,T,C] -> [B,C,Tout] with `pad` at t >= lens[b]"""
    _chk(x, 'x'); _chk(lens, 'lens', torch.int64)
    B, T, C = x.shape
    assert lens.numel() == B
    out = torch.empty(B, C, Tout, device=x.device, dtype=x.dtype)
    _lib.call('ft_transpose_pad_lens_fwd', _p(x), _p(lens), _p(out), B, T, C, Tout, pad, _stream())
    return out


def transpose_pad_bwd(dout: torch.Tensor, T: int) -> torch.Tensor:
    _chk(dout, 'dout')
    B, C, Tout = dout.shape
    dx = torch.empty(B, T, C, device=dout.device, dtype=dout.dtype)
    _lib.call('ft_transpose_pad_bwd', _p(dout), _p(dx), B, T, C, Tout, _stream())
    return dx


def copy_segments(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor]) -> None:
    """dsts[i] <- srcs[i] (contiguous fp32, equal numel), all in one launch (at most 64 pairs per launch)."""
    for i in range(0, len(srcs), 64):
        ss, dd = srcs[i:i + 64], dsts[i:i + 64]
        n = len(ss)
        for a, b in zip(ss, dd):
            _chk(a, 'src'); _chk(b, 'dst')
            if a.numel() != b.numel():
                raise _lib.FtError('copy_segments: size mismatch')
        lens = (ctypes.c_long * n)(*[a.numel() for a in ss])
        _lib.call('ft_copy_segments', _ptr_array(ss), _ptr_array(dd), lens, n, _stream())


def transpose2d(x: torch.Tensor) -> torch.Tensor:
    """[R,C] -> [C,R] (used for W_hh^T in BPTT)."""
    R, C = x.shape
    if pack_cache is not None:
        hit = pack_cache.t2d.get((x.data_ptr(), R, C))
        if hit is not None:
            return hit
    return transpose_pad_fwd(x.view(1, R, C), R, 0.0).view(C, R)


def masked_l1_fwd(x: torch.Tensor, target: torch.Tensor, lens: torch.Tensor):
    _chk(x, 'x'); _chk(target, 'target'); _chk(lens, 'lens', torch.int64)
    B, C, T = x.shape
    loss = torch.empty((), device=x.device, dtype=x.dtype)
    inv = torch.empty(1, device=x.device, dtype=x.dtype)
    _lib.call('ft_masked_l1_fwd', _p(x), _p(target), _p(lens), _p(loss), _p(inv), B, C, T,
              *scratch('ft_masked_l1_workspace', device=x.device), _stream())
    return loss, inv


def masked_l1_bwd(x, target, lens, inv, grad_out: Optional[torch.Tensor], factor: float = 1.0) -> torch.Tensor:
    B, C, T = x.shape
    dx = torch.empty_like(x)
    _lib.call('ft_masked_l1_bwd', _p(x), _p(target), _p(lens), _p(inv), _p(grad_out), factor, _p(dx), B, C, T,
              _stream())
    return dx


# ---------------------------------------------------------------------------------------------------
# recurrences
# ---------------------------------------------------------------------------------------------------
# All recurrence buffers are TIME-major: xp [T,B,2*G*H], out / cstate [T,B,2H], gates [T,B,2,4H].
_rnn_ws = {}          # (device, stream, gates, B, H) -> workspace of the persistent recurrence kernels


def _rnn_workspace(gates: int, B: int, H: int, device):
    nbytes = _lib.query('ft_rnn_workspace', gates, B, H)
    if nbytes == 0:
        return None, 0
    key = (torch.device(device).index or 0, _stream(), gates, B, H)
    ws = _rnn_ws.get(key)
    if ws is None:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        _rnn_ws[key] = ws
    return ws, nbytes


def check_rnn_status(clear: bool = True) -> None:
    """Synchronises the device and raises if ANY persistent recurrence launched on it since the fault word was last
    cleared timed out (the word is sticky: later launches, successful or not, never reset it).  clear=True resets it, so
    that a caller who switches to the per-step kernels is not told about the same timeout again.  Training does not
    depend on anyone calling this: the optimizer kernels read the same word on the device and skip the update
    (trainer.TrainStep)."""
    _lib.call('ft_rnn_status', int(clear))


def rnn_note_join(waiting: 'torch.cuda.Stream', joined: 'torch.cuda.Stream') -> None:
    """call right after waiting.wait_stream(joined): see ft_rnn_note_join (include/fwdtaco_hip.h)"""
    _lib.call('ft_rnn_note_join', waiting.cuda_stream, joined.cuda_stream)


def rnn_mode_counts():
    """((direction, batch group) groups that ran XCD-local, groups on the agent-scope protocol) since load; syncs"""
    a, b = ctypes.c_long(0), ctypes.c_long(0)
    _lib.call('ft_rnn_mode_counts', ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def rnn_counters():
    """(launches that ran in the persistent form, launches that cannot fit the chip -> per-step kernels) since load"""
    a, b = ctypes.c_long(0), ctypes.c_long(0)
    _lib.call('ft_rnn_counters', ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def rnn_waited_launches() -> int:
    """persistent launches whose stream first had to wait (on the device) for another stream's persistent launches"""
    return int(_lib.query('ft_rnn_waited_launches'))


RNN_PLAN_KINDS = ('per-step', 'fwd', 'bwd', 'bwd_rs')


def rnn_plan(gates: int, backward: bool, B: int, T: int, H: int, nd: int = 2):
    """ft_rnn_plan (include/fwdtaco_hip.h): the persistent form this recurrence would take under the current FT_RNN_*
    environment, decided on the host alone; None where the per-step kernels would run.  tag is the kernel as the
    FT_RNN_DEBUG line names it; aligned / spread: workgroups per XCD slot in that layout, 0 where it does not apply."""
    f = (ctypes.c_long * 16)()
    _lib.call('ft_rnn_plan', gates, int(backward), B, T, H, nd, f)
    if f[0] == 0:
        return None
    keys = ('threads', 'rows', 'nchunks', 'groups', 'total', 'aligned', 'spread', 'granules', 'workspace')
    return dict(zip(keys, f[7:]), kind=RNN_PLAN_KINDS[f[0]], tag=f'{RNN_PLAN_KINDS[f[0]]}<{",".join(map(str, f[1:7]))}>')


def gru_fwd(xp, whh_f, whh_r, bhh_f, bhh_r, H: int, save_gates: bool):
    _chk(xp, 'xp')
    T, B, _ = xp.shape
    out = torch.empty(T, B, 2 * H, device=xp.device, dtype=xp.dtype)
    gates = torch.empty(T, B, 2, 4 * H, device=xp.device, dtype=xp.dtype) if save_gates else None
    ws, nb = _rnn_workspace(3, B, H, xp.device)
    _lib.call('ft_gru_fwd', _p(xp), _p(whh_f), _p(whh_r), _p(bhh_f), _p(bhh_r), _p(out), _p(gates), B, T, H,
              _p(ws), nb, _stream())
    return out, gates


def gru_fwd_lens(xp, whh_f, whh_r, bhh_f, bhh_r, lens: torch.Tensor, H: int):
    """gru_fwd over a packed batch: item b runs lens[b] steps (reverse from lens[b] - 1), out is zero beyond"""
    _chk(xp, 'xp'); _chk(lens, 'lens', torch.int64)
    T, B, _ = xp.shape
    assert lens.numel() == B
    out = torch.empty(T, B, 2 * H, device=xp.device, dtype=xp.dtype)
    ws, nb = _rnn_workspace(3, B, H, xp.device)
    _lib.call('ft_gru_fwd_lens', _p(xp), _p(whh_f), _p(whh_r), _p(bhh_f), _p(bhh_r), _p(lens), _p(out), None, B, T, H,
              _p(ws), nb, _stream())
    return out


def gru_bwd(dout, out, gates, whhT_f, whhT_r, H: int):
    _chk(dout, 'dout')
    T, B, _ = out.shape
    dxp = torch.empty(T, B, 6 * H, device=out.device, dtype=out.dtype)
    dhp = torch.empty(T, B, 6 * H, device=out.device, dtype=out.dtype)
    carry = torch.empty(B, 2, H, device=out.device, dtype=out.dtype)
    ws, nb = _rnn_workspace(3, B, H, out.device)
    _lib.call('ft_gru_bwd', _p(dout), _p(out), _p(gates), _p(whhT_f), _p(whhT_r), _p(dxp), _p(dhp), _p(carry), B, T,
              H, _p(ws), nb, _stream())
    return dxp, dhp


def lstm_fwd(xp, whh_f, whh_r, bhh_f, bhh_r, lens: Optional[torch.Tensor], H: int, save_gates: bool):
    _chk(xp, 'xp')
    T, B, _ = xp.shape
    raw = torch.empty(T, B, 2 * H, device=xp.device, dtype=xp.dtype)
    cst = torch.empty(T, B, 2 * H, device=xp.device, dtype=xp.dtype)
    gates = torch.empty(T, B, 2, 4 * H, device=xp.device, dtype=xp.dtype) if save_gates else None
    ws, nb = _rnn_workspace(4, B, H, xp.device)
    _lib.call('ft_lstm_fwd', _p(xp), _p(whh_f), _p(whh_r), _p(bhh_f), _p(bhh_r), _p(lens), _p(raw), _p(cst),
              _p(gates), B, T, H, _p(ws), nb, _stream())
    return raw, cst, gates


# ---- recurrent layer forward with the input projection overlapped with the recurrence (ft_*_layer_fwd) ----
_proj_streams = {}


def rnn_overlap(rows: int, T: int) -> int:
    """number of time chunks the input projection of a recurrent layer is cut into (0: projection in front, whole).
    Off by default: measured neutral on the train step (the only layer it applies to, the postnet GRU, has a 130 us
    projection; the 512-wide LSTM fills its XCDs and cannot be overlapped from another stream at all,
    profiles/r03_xcd_dispatch_probe.txt).  FT_RNN_OVERLAP=1 turns it on, FT_RNN_CHUNKS sets the count (default 4)."""
    if os.environ.get('FT_RNN_OVERLAP', '0') != '1' or rows < 8192 or T < 256:
        return 0
    return max(2, int(os.environ.get('FT_RNN_CHUNKS', '4')))


def _proj_stream(device) -> 'torch.cuda.Stream':
    key = torch.device(device).index or 0
    st = _proj_streams.get(key)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _proj_streams[key] = st
    return st


def lstm_layer_fwd(x, wih_f, wih_r, bih_f, bih_r, whh_f, whh_r, bhh_f, bhh_r, lens: Optional[torch.Tensor], H: int,
                   save_gates: bool, nchunks: int):
    """x [B,T,I] batch-major -> (raw, cst, gates) as lstm_fwd; the projection runs in time chunks beside the recurrence"""
    _chk(x, 'x')
    B, T, I = x.shape
    dev = x.device
    xp = torch.empty(T, B, 8 * H, device=dev, dtype=x.dtype)
    raw = torch.empty(T, B, 2 * H, device=dev, dtype=x.dtype)
    cst = torch.empty(T, B, 2 * H, device=dev, dtype=x.dtype)
    gates = torch.empty(T, B, 2, 4 * H, device=dev, dtype=x.dtype) if save_gates else None
    gate = torch.empty(16, device=dev, dtype=torch.int32)
    ws, nb = _rnn_workspace(4, B, H, dev)
    lead = int(os.environ.get('FT_RNN_REV_LEAD', str(nchunks // 2))) if lens is not None else 0
    _lib.call('ft_lstm_layer_fwd', _p(x), I, _p(wih_f), _p(wih_r), _p(bih_f), _p(bih_r), _p(xp), _p(whh_f), _p(whh_r),
              _p(bhh_f), _p(bhh_r), _p(lens), _p(raw), _p(cst), _p(gates), B, T, H, _p(ws), nb, _p(gate), nchunks, lead,
              _stream(), _proj_stream(dev).cuda_stream)
    return raw, cst, gates


def gru_layer_fwd(x, wih_f, wih_r, bih_f, bih_r, whh_f, whh_r, bhh_f, bhh_r, H: int, save_gates: bool, nchunks: int):
    _chk(x, 'x')
    B, T, I = x.shape
    dev = x.device
    xp = torch.empty(T, B, 6 * H, device=dev, dtype=x.dtype)
    out = torch.empty(T, B, 2 * H, device=dev, dtype=x.dtype)
    gates = torch.empty(T, B, 2, 4 * H, device=dev, dtype=x.dtype) if save_gates else None
    gate = torch.empty(16, device=dev, dtype=torch.int32)
    ws, nb = _rnn_workspace(3, B, H, dev)
    _lib.call('ft_gru_layer_fwd', _p(x), I, _p(wih_f), _p(wih_r), _p(bih_f), _p(bih_r), _p(xp), _p(whh_f), _p(whh_r),
              _p(bhh_f), _p(bhh_r), _p(out), _p(gates), B, T, H, _p(ws), nb, _p(gate), nchunks, _stream(),
              _proj_stream(dev).cuda_stream)
    return out, gates


def gru_layer_fwd_lens(x, wih_f, wih_r, bih_f, bih_r, whh_f, whh_r, bhh_f, bhh_r, lens: torch.Tensor, H: int,
                       nchunks: int):
    """gru_layer_fwd over a packed batch (gru_fwd_lens)"""
    _chk(x, 'x'); _chk(lens, 'lens', torch.int64)
    B, T, I = x.shape
    assert lens.numel() == B
    dev = x.device
    xp = torch.empty(T, B, 6 * H, device=dev, dtype=x.dtype)
    out = torch.empty(T, B, 2 * H, device=dev, dtype=x.dtype)
    gate = torch.empty(16, device=dev, dtype=torch.int32)
    ws, nb = _rnn_workspace(3, B, H, dev)
    lead = int(os.environ.get('FT_RNN_REV_LEAD', str(nchunks // 2)))
    _lib.call('ft_gru_layer_fwd_lens', _p(x), I, _p(wih_f), _p(wih_r), _p(bih_f), _p(bih_r), _p(xp), _p(whh_f),
              _p(whh_r), _p(bhh_f), _p(bhh_r), _p(lens), _p(out), None, B, T, H, _p(ws), nb, _p(gate), nchunks, lead,
              _stream(), _proj_stream(dev).cuda_stream)
    return out


def lstm_bwd(dout, raw, cst, gates, whhT_f, whhT_r, lens: Optional[torch.Tensor], H: int):
    _chk(dout, 'dout')
    T, B, _ = raw.shape
    dg = torch.empty(T, B, 8 * H, device=raw.device, dtype=raw.dtype)
    carry = torch.empty(B, 2, H, device=raw.device, dtype=raw.dtype)
    ws, nb = _rnn_workspace(4, B, H, raw.device)
    _lib.call('ft_lstm_bwd', _p(dout), _p(raw), _p(cst), _p(gates), _p(whhT_f), _p(whhT_r), _p(lens), _p(dg),
              _p(carry), B, T, H, _p(ws), nb, _stream())
    return dg


def fill_padded(raw_tm: torch.Tensor, lens: Optional[torch.Tensor], pad: float) -> torch.Tensor:
    """time-major raw [T,B,C] -> batch-major [B,T,C] with `pad` at t >= lens[b] (lens None: pure layout change)"""
    T, B, C = raw_tm.shape
    out = torch.empty(B, T, C, device=raw_tm.device, dtype=raw_tm.dtype)
    _lib.call('ft_fill_padded', _p(raw_tm), _p(lens), _p(out), B, T, C, pad, _stream())
    return out


def bt_transpose(src: torch.Tensor, to_time_major: bool) -> torch.Tensor:
    """[B,T,C] -> [T,B,C] (to_time_major) or [T,B,C] -> [B,T,C]"""
    _chk(src, 'src')
    if to_time_major:
        B, T, C = src.shape
        dst = torch.empty(T, B, C, device=src.device, dtype=src.dtype)
    else:
        T, B, C = src.shape
        dst = torch.empty(B, T, C, device=src.device, dtype=src.dtype)
    _lib.call('ft_bt_transpose', _p(src), _p(dst), B, T, C, int(to_time_major), _stream())
    return dst


def mask_rows(src: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    B, T, C = src.shape
    dst = torch.empty_like(src)
    _lib.call('ft_mask_rows', _p(src), _p(lens), _p(dst), B, T, C, _stream())
    return dst


# ---------------------------------------------------------------------------------------------------
# audio front end (csrc/ft_audio.hip; the public interface is forwardtacotron_amd/audio.py)
# ---------------------------------------------------------------------------------------------------
def wav_trim_peak(wav: torch.Tensor, lens: torch.Tensor, Lmax: int, do_trim: bool, top_db: float, peak_mode: int,
                  hop: int, alloc=torch.empty):
    """wav [B, ld] fp32, lens [B] int64 (device) -> dict of per-item device tensors: trim_start, trim_end, wav_len,
    mel_len (int64), peak (fp32), scaled (int32).  peak_mode: 1 always scale, 0 only if peak > 1, -1 never."""
    _chk(wav, 'wav'); _chk(lens, 'lens', torch.int64)
    B, ld = wav.shape
    dev = wav.device
    out = {k: alloc(B, dtype=torch.int64, device=dev) for k in ('trim_start', 'trim_end', 'wav_len', 'mel_len')}
    out['peak'] = alloc(B, dtype=torch.float32, device=dev)
    out['scaled'] = alloc(B, dtype=torch.int32, device=dev)
    ws = workspace(_lib.query('ft_wav_trim_peak_workspace', B, Lmax), dev)
    _lib.call('ft_wav_trim_peak', _p(wav), ld, _p(lens), B, Lmax, int(do_trim), float(top_db), int(peak_mode), hop,
              _p(out['trim_start']), _p(out['trim_end']), _p(out['wav_len']), _p(out['mel_len']), _p(out['peak']),
              _p(out['scaled']), _p(ws), _stream())
    return out


def wav_pack(wav: torch.Tensor, tp, stride: int, n_fft: int, reflect: bool, alloc=torch.empty):
    """-> (packed [B * stride + n_fft], wav_out [B, ld]); tp = the dict wav_trim_peak returned"""
    B, ld = wav.shape
    packed = alloc(B * stride + n_fft, dtype=torch.float32, device=wav.device)
    wav_out = alloc(B, ld, dtype=torch.float32, device=wav.device)
    _lib.call('ft_wav_pack', _p(wav), ld, _p(tp['trim_start']), _p(tp['trim_end']), _p(tp['peak']), _p(tp['scaled']), B,
              _p(packed), stride, n_fft, int(reflect), _p(wav_out), ld, _stream())
    return packed, wav_out


def mel_project(spec: torch.Tensor, Fp: int, rows_per_item: int, mel_len: torch.Tensor, w: torch.Tensor,
                meta: torch.Tensor, n_mels: int, B: int, Tmax: int, log_clip: bool, pad_value: float,
                alloc=torch.empty) -> torch.Tensor:
    """split spectra [B * rows_per_item, 2 Fp] -> (log-)mel [B, n_mels, Tmax], pad_value at t >= mel_len[b]"""
    _chk(spec, 'spec'); _chk(mel_len, 'mel_len', torch.int64); _chk(w, 'w'); _chk(meta, 'meta', torch.int32)
    mel = alloc(B, n_mels, Tmax, dtype=torch.float32, device=spec.device)
    _lib.call('ft_mel_project', _p(spec), spec.shape[1], Fp, rows_per_item, _p(mel_len), _p(w), _p(meta), w.numel(),
              n_mels, B, Tmax, int(log_clip), float(pad_value), _p(mel), _stream())
    return mel


def resample_poly_ragged(x: torch.Tensor, lens: torch.Tensor, Lmax: int, tab: Optional[torch.Tensor], up: int, down: int,
                         half: int, ldy: int, err: Optional[torch.Tensor] = None, alloc=torch.empty):
    """csrc/ft_resample.hip: x [B, ldx] fp32, lens [B] int64 (device), tab = the phase-major coefficient table (None for
    up == down) -> (y [B, ldy] fp32, zero at j >= out_len[b]; out_len [B] int64 = ceil(lens * up / down))"""
    _chk(x, 'wav'); _chk(lens, 'wav_len', torch.int64)
    if tab is not None:
        _chk(tab, 'tab')
    B, ldx = x.shape
    y = alloc(B, ldy, dtype=torch.float32, device=x.device)
    out_len = alloc(B, dtype=torch.int64, device=x.device)
    _lib.call('ft_resample_poly_ragged', _p(x), ldx, _p(lens), B, Lmax, _p(tab), up, down, half, _p(y), ldy, _p(out_len),
              _p(err), _stream())
    return y, out_len


# ---------------------------------------------------------------------------------------------------
# pYIN on a ragged batch (csrc/ft_pitch.hip; the public interface is pitch.LibrosaPitchExtractor).  `tb` is
# pitch.pyin_tables(...), `dev` its float32 tables on the device.
# ---------------------------------------------------------------------------------------------------
def pyin_cmnd(wav: torch.Tensor, lens: torch.Tensor, Lmax: int, frame_length: int, hop: int, pmin: int, pmax: int,
              Tmax: int, alloc=torch.empty):
    """wav [B, ld] fp32, lens [B] int64 (device) -> (dn [B, Tmax, P] fp32, frames [B] int64 = 1 + lens // hop)"""
    _chk(wav, 'wav'); _chk(lens, 'wav_len', torch.int64)
    B, ld = wav.shape
    dn = alloc(B, Tmax, pmax - pmin + 1, dtype=torch.float32, device=wav.device)
    frames = alloc(B, dtype=torch.int64, device=wav.device)
    _lib.call('ft_pyin_cmnd', _p(wav), ld, _p(lens), B, Lmax, frame_length, hop, pmin, pmax, Tmax, _p(dn), _p(frames),
              _stream())
    return dn, frames


def pyin_observe(dn: torch.Tensor, frames: torch.Tensor, tb, dev, debug: bool = False, alloc=torch.empty):
    """dn [B, Tmax, P], frames [B] int64 -> {'lo_v' [B, Tmax, N], 'lo_u', 'vp' [B, Tmax]}; debug adds 'prob' [B, Tmax, P],
    'info' [B, Tmax, 102] int32 and 'pos' [B, Tmax, P, 100] int16 (include/fwdtaco_hip.h: ft_pyin_observe)"""
    _chk(dn, 'dn'); _chk(frames, 'frames', torch.int64)
    B, Tmax, P = dn.shape
    if P != tb['P']:
        raise _lib.FtError(f'pyin_observe: dn holds {P} periods, the tables {tb["P"]}')
    N = tb['N']
    out = {'lo_v': alloc(B, Tmax, N, dtype=torch.float32, device=dn.device),
           'lo_u': alloc(B, Tmax, dtype=torch.float32, device=dn.device),
           'vp': alloc(B, Tmax, dtype=torch.float32, device=dn.device)}
    if debug:
        out['prob'] = alloc(B, Tmax, P, dtype=torch.float32, device=dn.device)
        out['info'] = alloc(B, Tmax, 102, dtype=torch.int32, device=dn.device)
        out['pos'] = alloc(B, Tmax, P, 100, dtype=torch.int16, device=dn.device)
    _lib.call('ft_pyin_observe', _p(dn), _p(frames), B, Tmax, P, tb['pmin'], N, float(tb['sr']), float(tb['fmin']),
              _p(dev['thr']), _p(dev['bp']), _p(dev['bpc']), _p(dev['E']), _p(dev['C']), tb['nE'], tb['LZ'],
              _p(out['lo_v']), _p(out['lo_u']), _p(out['vp']), _p(out.get('prob')), _p(out.get('info')), _p(out.get('pos')), _stream())
    return out


def pyin_viterbi(lo_v: torch.Tensor, lo_u: torch.Tensor, frames: torch.Tensor, tb, dev, alloc=torch.empty):
    """lo_v [B, Tmax, N], lo_u [B, Tmax], frames [B] int64 -> {'state' [B, Tmax] int32, 'score' [B], 'pitch' [B, Tmax]}"""
    _chk(lo_v, 'lo_v'); _chk(lo_u, 'lo_u'); _chk(frames, 'frames', torch.int64)
    B, Tmax, N = lo_v.shape
    if N != tb['N'] or lo_u.shape != (B, Tmax):
        raise _lib.FtError('pyin_viterbi: lo_v must be [B, Tmax, N] of the tables and lo_u [B, Tmax]')
    out = {'state': alloc(B, Tmax, dtype=torch.int32, device=lo_v.device),
           'score': alloc(B, dtype=torch.float32, device=lo_v.device),
           'pitch': alloc(B, Tmax, dtype=torch.float32, device=lo_v.device)}
    nbytes = _lib.query('ft_pyin_viterbi_workspace', B, Tmax, N)
    ws = alloc(max(nbytes, 2), dtype=torch.uint8, device=lo_v.device)
    _lib.call('ft_pyin_viterbi', _p(lo_v), _p(lo_u), _p(frames), B, Tmax, N, tb['half'], _p(dev['logtri']),
              _p(dev['lognorm']), _p(dev['freqs']), tb['ls'], tb['lw'], tb['LZ'], tb['lN'], _p(out['state']),
              _p(out['score']), _p(out['pitch']), _p(ws), nbytes, _stream())
    return out


# ---------------------------------------------------------------------------------------------------
# Griffin-Lim on a ragged batch (csrc/ft_dsp.hip, the *_ragged entries; the public interface is
# vocoder.GriffinLim.griffinlim_batch).  Item b owns rows [b * Tcap, (b + 1) * Tcap); mel_len int64 [B] on the device.
# ---------------------------------------------------------------------------------------------------
def gl_exp_transpose_ragged(mel: torch.Tensor, mel_len: torch.Tensor, Tcap: int, err: Optional[torch.Tensor] = None,
                            alloc=torch.empty) -> torch.Tensor:
    """log-mel [B, C, Tmax] -> exp, frames-major [B * Tcap, C]; rows n >= mel_len[b] are zero"""
    _chk(mel, 'mel'); _chk(mel_len, 'mel_len', torch.int64)
    B, C, Tmax = mel.shape
    out = alloc(B * Tcap, C, dtype=torch.float32, device=mel.device)
    _lib.call('ft_gl_exp_transpose_ragged', _p(mel), _p(mel_len), _p(out), B, C, Tmax, Tcap, _p(err), _stream())
    return out


def gl_relu(x: torch.Tensor) -> torch.Tensor:
    """x = max(x, 0) in place"""
    _chk(x, 'x')
    _lib.call('ft_gl_relu', _p(x), x.numel(), _stream())
    return x


def gl_init_ragged(S: torch.Tensor, mel_len: torch.Tensor, B: int, Tcap: int, Tmax: int,
                   u: Optional[torch.Tensor] = None, seed: int = 0, err: Optional[torch.Tensor] = None,
                   want_u: bool = False, alloc=torch.empty):
    """S [B * Tcap, Fp] -> proj [B * Tcap, 2 Fp] = S exp(2 pi i u), zero rows at n >= mel_len[b]; u given, or drawn on the
    device from (seed, n, m).  want_u: also return the u that was used -> (proj, u)"""
    _chk(S, 'S'); _chk(mel_len, 'mel_len', torch.int64)
    rows, Fp = S.shape
    if rows != B * Tcap or (u is not None and tuple(u.shape) != (rows, Fp)):
        raise _lib.FtError(f'gl_init_ragged: S (and init_u) must be [B * Tcap = {B * Tcap}, Fp], got {tuple(S.shape)}'
                           + ('' if u is None else f' and {tuple(u.shape)}'))
    if u is not None:
        _chk(u, 'init_u')
    proj = alloc(rows, 2 * Fp, dtype=torch.float32, device=S.device)
    u_out = alloc(rows, Fp, dtype=torch.float32, device=S.device) if want_u else None
    _lib.call('ft_gl_init_ragged', _p(u), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(S), _p(mel_len), _p(proj), _p(u_out), B,
              Tcap, Tmax, Fp, _p(err), _stream())
    return (proj, u_out) if want_u else proj


def gl_phase_ragged(rebuilt: torch.Tensor, tprev: torch.Tensor, S: torch.Tensor, mel_len: torch.Tensor,
                    proj: torch.Tensor, B: int, Tcap: int, Tmax: int, alpha: float, has_prev: bool) -> None:
    """the fast Griffin-Lim update in place on proj / tprev [B * Tcap, 2 Fp]; rows n >= mel_len[b] become zero"""
    _lib.call('ft_gl_phase_ragged', _p(rebuilt), _p(tprev), _p(S), _p(mel_len), _p(proj), B, Tcap, Tmax, S.shape[1],
              float(alpha), int(has_prev), _stream())


def overlap_add_ragged(frames: torch.Tensor, w2: torch.Tensor, mel_len: torch.Tensor, B: int, Tcap: int, Tmax: int,
                       n_fft: int, hop: int, as_wav: bool = False, alloc=torch.empty) -> torch.Tensor:
    """frames [B * Tcap, n_fft] -> the packed padded signals [B * Tcap * hop + n_fft] (the next STFT's operand), or with
    as_wav the signals themselves [B, hop * (Tmax - 1)], zero beyond hop * (mel_len[b] - 1)"""
    if as_wav:
        out = alloc(B, hop * (Tmax - 1), dtype=torch.float32, device=frames.device)
    else:
        out = alloc(B * Tcap * hop + n_fft, dtype=torch.float32, device=frames.device)
    if out.numel():                            # Tmax == 1: every wav is empty
        _lib.call('ft_overlap_add_ragged', _p(frames), _p(w2), _p(mel_len), None if as_wav else _p(out),
                  _p(out) if as_wav else None, B, Tcap, Tmax, n_fft, hop, _stream())
    return out


# ---------------------------------------------------------------------------------------------------
# speaker embeddings (csrc/ft_speaker.hip; the public interface is speaker.VoiceEncoder)
# ---------------------------------------------------------------------------------------------------
def spk_slices(n: int, hop: int, partial_frames: int, frame_step: int, cov_num: int, cov_den: int):
    """(count, frames) of the slice rule at a length of n samples: the function the kernels apply on the device, on the
    host (no device needed)"""
    a, b = ctypes.c_long(0), ctypes.c_long(0)
    _lib.call('ft_spk_slices', n, hop, partial_frames, frame_step, cov_num, cov_den, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def lstm_fwd_uni(xp: torch.Tensor, whh: torch.Tensor, bhh: torch.Tensor, H: int, alloc=torch.empty):
    """one direction from zero states: xp [T, B, 4H] (x W_ih^T + b_ih, time-major) -> (out_raw, cstate) [T, B, H]"""
    _chk(xp, 'xp'); _chk(whh, 'whh'); _chk(bhh, 'bhh')
    T, B, _ = xp.shape
    out = alloc(T, B, H, dtype=torch.float32, device=xp.device)
    cst = alloc(T, B, H, dtype=torch.float32, device=xp.device)
    ws, nb = _rnn_workspace(4, B, H, xp.device)
    _lib.call('ft_lstm_fwd_uni', _p(xp), _p(whh), _p(bhh), _p(out), _p(cst), B, T, H, _p(ws), nb, _stream())
    return out, cst


def spk_gain(wav: torch.Tensor, lens: torch.Tensor, Lmax: int, target: float, hop: int, partial_frames: int,
             frame_step: int, cov_num: int, cov_den: int, normalize: bool, err: Optional[torch.Tensor] = None,
             alloc=torch.empty):
    """wav [B, ld] fp32, lens [B] int64 (device) -> (gain [B] fp32, n_partials [B] int64, frames [B] int64)"""
    _chk(wav, 'wav'); _chk(lens, 'wav_len', torch.int64)
    B, ld = wav.shape
    gain = alloc(B, dtype=torch.float32, device=wav.device)
    n_partials = alloc(B, dtype=torch.int64, device=wav.device)
    frames = alloc(B, dtype=torch.int64, device=wav.device)
    _lib.call('ft_spk_gain', _p(wav), ld, _p(lens), B, Lmax, float(target), hop, partial_frames, frame_step, cov_num,
              cov_den, int(normalize), _p(gain), _p(n_partials), _p(frames), _p(err), _stream())
    return gain, n_partials, frames


def spk_pack(wav: torch.Tensor, lens: torch.Tensor, Lmax: int, gain: torch.Tensor, stride: int, n_fft: int,
             alloc=torch.empty) -> torch.Tensor:
    """-> packed [B * stride + n_fft]: gain * wav behind n_fft / 2 zeros, zero-extended, one stride per item"""
    B, ld = wav.shape
    packed = alloc(B * stride + n_fft, dtype=torch.float32, device=wav.device)
    _lib.call('ft_spk_pack', _p(wav), ld, _p(lens), B, Lmax, _p(gain), _p(packed), stride, n_fft, _stream())
    return packed


def spk_mel_power(spec: torch.Tensor, Fp: int, rows_per_item: int, frames: torch.Tensor, w: torch.Tensor,
                  meta: torch.Tensor, n_mels: int, B: int, alloc=torch.empty) -> torch.Tensor:
    """split spectra [B * rows_per_item, 2 Fp] -> power mel [B * rows_per_item, n_mels], zero rows at t >= frames[b]"""
    _chk(spec, 'spec'); _chk(frames, 'frames', torch.int64); _chk(w, 'w'); _chk(meta, 'meta', torch.int32)
    mel = alloc(B * rows_per_item, n_mels, dtype=torch.float32, device=spec.device)
    _lib.call('ft_spk_mel_power', _p(spec), spec.shape[1], Fp, rows_per_item, _p(frames), _p(w), _p(meta), w.numel(),
              n_mels, B, _p(mel), _stream())
    return mel


def spk_gather_partials(mel: torch.Tensor, rows_per_item: int, frames: torch.Tensor, table: torch.Tensor, p0: int,
                        P: int, partial_frames: int, B: int, alloc=torch.empty) -> torch.Tensor:
    """slots p0 .. p0 + P - 1 of table [*, 2] int32 = (item, first frame) -> [partial_frames, P, n_mels] time-major"""
    _chk(mel, 'mel'); _chk(table, 'table', torch.int32)
    assert 0 <= p0 and p0 + P <= table.shape[0]
    n_mels = mel.shape[1]
    out = alloc(partial_frames, P, n_mels, dtype=torch.float32, device=mel.device)
    _lib.call('ft_spk_gather_partials', _p(mel), rows_per_item, n_mels, _p(frames), table.data_ptr() + 8 * p0, P,
              partial_frames, B, _p(out), _stream())
    return out


def spk_segment_mean_norm(rows: torch.Tensor, index: Optional[torch.Tensor], offsets: torch.Tensor,
                          count: Optional[torch.Tensor], normalize_rows: bool, rows_out: Optional[torch.Tensor] = None,
                          alloc=torch.empty) -> torch.Tensor:
    """rows [N, E], offsets int64 [S + 1] (into index int64, or into the rows themselves) -> [S, E] unit mean rows"""
    _chk(rows, 'rows'); _chk(offsets, 'offsets', torch.int64)
    N, E = rows.shape
    S = offsets.numel() - 1
    if index is not None:
        _chk(index, 'index', torch.int64)
    if count is not None:
        _chk(count, 'count', torch.int64)
        assert count.numel() == S
    out = alloc(S, E, dtype=torch.float32, device=rows.device)
    _lib.call('ft_spk_segment_mean_norm', _p(rows), N, E, _p(index), _p(offsets), _p(count), S, int(normalize_rows),
              _p(out), _p(rows_out), _stream())
    return out


# ---------------------------------------------------------------------------------------------------
# Tacotron teacher training (csrc/ft_taco_train.hip)
# ---------------------------------------------------------------------------------------------------
def taco_attend_bwd(ep: torch.Tensor, epq: torch.Tensor, P: torch.Tensor, w_ih: torch.Tensor, w_hh: torch.Tensor,
                    b_hh: torch.Tensor, W: torch.Tensor, bW: torch.Tensor, cw: torch.Tensor, L: torch.Tensor,
                    bL: torch.Tensor, v: torch.Tensor, hist: torch.Tensor, attn: torch.Tensor, dhist: torch.Tensor,
                    ws: Optional[torch.Tensor] = None, alloc=torch.empty) -> dict:
    """backward of ft_taco_attend from dhist [S,B,512] -> dict of dep, depq [B,Tx,256], dP [S,B,768], dw_ih_ctx [768,256]
    (the gradient of w_ih[:, :256]; w_ih is [768, >= 256], only those columns are read), dw_hh, db_hh, dW, dbW, dcw, dL,
    dbL, dv.  ws: a byte buffer of at least ft_taco_attend_bwd_workspace(B, Tx, S), or None for the stream's own."""
    for n, t in (('ep', ep), ('epq', epq), ('P', P), ('w_ih', w_ih), ('w_hh', w_hh), ('b_hh', b_hh), ('W', W), ('bW', bW),
                 ('cw', cw), ('L', L), ('bL', bL), ('v', v), ('hist', hist), ('attn', attn), ('dhist', dhist)):
        _chk(t, n)
    B, Tx, D = ep.shape
    S = P.shape[0]
    if (D != 256 or epq.shape != ep.shape or tuple(P.shape) != (S, B, 3 * D) or tuple(hist.shape) != (S, B, 2 * D)
            or dhist.shape != hist.shape or tuple(attn.shape) != (B, S, Tx)):
        raise _lib.FtError(f'taco_attend_bwd: inconsistent shapes ep {tuple(ep.shape)}, epq {tuple(epq.shape)}, P '
                           f'{tuple(P.shape)}, hist {tuple(hist.shape)}, dhist {tuple(dhist.shape)}, attn {tuple(attn.shape)}')
    nbytes = _lib.query('ft_taco_attend_bwd_workspace', B, Tx, S)
    if nbytes == 0:
        raise _lib.FtError(f'taco_attend_bwd: B >= 1, 1 <= Tx <= 1024 and S >= 1 are required (got B = {B}, Tx = {Tx}, '
                           f'S = {S})')
    if ws is None:
        ws = workspace(nbytes, ep.device)
    f32 = dict(dtype=torch.float32, device=ep.device)
    out = dict(dep=alloc(B, Tx, D, **f32), depq=alloc(B, Tx, D, **f32), dP=alloc(S, B, 3 * D, **f32),
               dw_ih_ctx=alloc(3 * D, D, **f32), dw_hh=alloc(3 * D, D, **f32), db_hh=alloc(3 * D, **f32),
               dW=alloc(D, D, **f32), dbW=alloc(D, **f32), dcw=alloc(*cw.shape, **f32), dL=alloc(*L.shape, **f32),
               dbL=alloc(D, **f32), dv=alloc(D, **f32))
    _lib.call('ft_taco_attend_bwd', _p(ep), _p(epq), _p(P), _p(w_ih), w_ih.shape[1], _p(w_hh), _p(b_hh), _p(W), _p(bW),
              _p(cw), _p(L), _p(bL), _p(v), _p(hist), _p(attn), _p(dhist), _p(out['dep']), _p(out['depq']), _p(out['dP']),
              _p(out['dw_ih_ctx']), _p(out['dw_hh']), _p(out['db_hh']), _p(out['dW']), _p(out['dbW']), _p(out['dcw']),
              _p(out['dL']), _p(out['dbL']), _p(out['dv']), B, Tx, S, _p(ws), ws.numel(), _stream())
    return out


def taco_lstm_zone_fwd(xp: torch.Tensor, w_hh: torch.Tensor, b_hh: torch.Tensor, p: float, seed: int,
                       alloc=torch.empty):
    """nn.LSTMCell over the S steps of xp [S,B,4L] (x W_ih^T + b_ih) from zero states with zoneout p (mask of
    ft_dropout(p, seed) over [S,B,L]: zoned where it is 0) -> (gates [S,B,4L] activated, c [S,B,L], zoned h [S,B,L])"""
    _chk(xp, 'xp'); _chk(w_hh, 'w_hh'); _chk(b_hh, 'b_hh')
    S, B, G = xp.shape
    L = w_hh.shape[1]
    if G != 4 * L or tuple(w_hh.shape) != (4 * L, L) or b_hh.numel() != 4 * L:
        raise _lib.FtError(f'taco_lstm_zone_fwd: xp {tuple(xp.shape)}, w_hh {tuple(w_hh.shape)}, b_hh {tuple(b_hh.shape)}')
    f32 = dict(dtype=torch.float32, device=xp.device)
    gates, c, h = alloc(S, B, G, **f32), alloc(S, B, L, **f32), alloc(S, B, L, **f32)
    _lib.call('ft_taco_lstm_zone_fwd', _p(xp), _p(w_hh), _p(b_hh), float(p), int(seed), _p(gates), _p(c), _p(h), B, S, L,
              _stream())
    return gates, c, h


def taco_lstm_zone_bwd(dout: torch.Tensor, gates: torch.Tensor, c: torch.Tensor, w_hhT: torch.Tensor, p: float,
                       seed: int, ws: Optional[torch.Tensor] = None, alloc=torch.empty) -> torch.Tensor:
    """dout [S,B,L] = the gradient of the zoned h; w_hhT [L,4L] -> dxp [S,B,4L], the gradient of the pre-activations"""
    _chk(dout, 'dout'); _chk(gates, 'gates'); _chk(c, 'c'); _chk(w_hhT, 'w_hhT')
    S, B, L = dout.shape
    if tuple(gates.shape) != (S, B, 4 * L) or c.shape != dout.shape or tuple(w_hhT.shape) != (L, 4 * L):
        raise _lib.FtError(f'taco_lstm_zone_bwd: dout {tuple(dout.shape)}, gates {tuple(gates.shape)}, c '
                           f'{tuple(c.shape)}, w_hhT {tuple(w_hhT.shape)}')
    nbytes = _lib.query('ft_taco_lstm_zone_workspace', B, L)
    if ws is None:
        ws = workspace(nbytes, dout.device)
    dxp = alloc(S, B, 4 * L, dtype=torch.float32, device=dout.device)
    _lib.call('ft_taco_lstm_zone_bwd', _p(dout), _p(gates), _p(c), _p(w_hhT), float(p), int(seed), _p(dxp), B, S, L,
              _p(ws), ws.numel(), _stream())
    return dxp


def relu_dropout_bwd(dy: torch.Tensor, y: torch.Tensor, p: float) -> torch.Tensor:
    """y = dropout(relu(z), p) as stored -> dz = y > 0 ? dy / (1 - p) : 0"""
    _chk(dy, 'dy'); _chk(y, 'y')
    dz = torch.empty_like(y)
    _lib.call('ft_relu_dropout_bwd', _p(dy), _p(y), _p(dz), y.numel(), float(p), _stream())
    return dz


def taco_mel_scatter(dwp: torch.Tensor, dw: torch.Tensor, n_mels: int, max_r: int, r: int) -> None:
    """dwp [r * n_mels, L] (rows k * n_mels + n) -> dw [n_mels * max_r, L] (rows n * max_r + k), zeros where k >= r"""
    _chk(dwp, 'dwp'); _chk(dw, 'dw')
    L = dw.shape[1]
    if tuple(dwp.shape) != (r * n_mels, L) or dw.shape[0] != n_mels * max_r:
        raise _lib.FtError(f'taco_mel_scatter: dwp {tuple(dwp.shape)}, dw {tuple(dw.shape)}, r = {r}')
    _lib.call('ft_taco_mel_scatter', _p(dwp), _p(dw), n_mels, max_r, r, L, _stream())


# ---------------------------------------------------------------------------------------------------
# The GAN vocoders on a ragged batch (csrc/ft_melgan.hip, ft_hifigan.hip; the public interfaces are melgan.MelGAN and
# hifigan.HiFiGAN).  Activations are channels-last [B * (Tmax + tail) * scale, C]; mel_len int64 [B] on the device, or
# None: every item has Tmax frames.  Weights and biases come packed from gan_vocoder.pack_*.  MelGAN reflects at an
# item's edges and carries `tail` appended frames; HiFi-GAN's edges are zeros and its tail is 0.  The three kernels both
# generators run have ONE wrapper each, taking the family; the melgan_* / hifigan_* names bind it.  Every limit and
# every choice of the launch plan is csrc/ft_voc_plan.h's, read through ft_voc_plan.
# ---------------------------------------------------------------------------------------------------
_MELGAN_KINDS = ('conv_in', 'upsample', 'resblock', 'conv_out')
_HIFIGAN_KINDS = ('conv_in', 'upsample', 'resconv', 'conv_out', 'respair')
_VOC_LIMITS = {'HIFIGAN_MAX_KERNEL': 0, 'HIFIGAN_MAX_HALO': 1, 'HIFIGAN_PAIR_HALO': 2}      # name -> ft_voc_plan field
_VOC_PAIR_IS_FUSED = 3
_pair_plan = {}


def __getattr__(name: str):
    """HIFIGAN_MAX_KERNEL (taps of a residual convolution), HIFIGAN_MAX_HALO (resconv: dilation * (k - 1) / 2 rows on
    either side of a tile) and HIFIGAN_PAIR_HALO (respair: the same for its first convolution), read from the library on
    first use: importing this module loads nothing"""
    if name in _VOC_LIMITS:
        value = globals()[name] = int(_lib.query('ft_voc_plan', _VOC_LIMITS[name], 0, 0, 0))
        return value
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def hifigan_pair_is_fused(width: int, k: int, d: int) -> bool:
    """the plan for ResBlock1's (convs1[m], convs2[m]): True = one ft_hifigan_respair launch with the intermediate in
    LDS, False = two launches of the residual convolution (the rule and its measurements: csrc/ft_voc_plan.h).  A pure
    function of its arguments, asked of the library once each"""
    key = (width, k, d)
    hit = _pair_plan.get(key)
    if hit is None:
        hit = _pair_plan[key] = bool(_lib.query('ft_voc_plan', _VOC_PAIR_IS_FUSED, int(width), int(k), int(d)))
    return hit


def melgan_tile_rows(kind: str, c: int) -> int:
    """rows per workgroup tile of the launch plan for width c: kind 'conv_in' (c = n_mels), 'upsample' (c = cin, input
    rows), 'resblock', 'conv_out' (samples); 0 where the width is not supported"""
    return int(_lib.query('ft_melgan_tile_rows', _MELGAN_KINDS.index(kind), int(c)))


def hifigan_tile_rows(kind: str, c: int) -> int:
    """rows per workgroup tile of the launch plan for width c: kind 'conv_in' (c = n_mels), 'upsample' (c = cin, input
    rows), 'resconv', 'conv_out' (samples), 'respair' (rows of the intermediate: a tile's output is that minus k - 1); 0
    where the width is not supported"""
    return int(_lib.query('ft_hifigan_tile_rows', _HIFIGAN_KINDS.index(kind), int(c)))


def _voc_conv_in(family, mel, mel_len, tail, pad_value, w, bias, cout, err, alloc):
    _chk(mel, 'mel'); _chk(w, 'w'); _chk(bias, 'bias')
    B, C, Tmax = mel.shape
    CP = -(-cout // 32) * 32
    if tuple(w.shape) != (7, C, CP) or bias.numel() != CP:
        raise _lib.FtError(f'{family}_conv_in: w {tuple(w.shape)} / bias {tuple(bias.shape)} for [7, {C}, {CP}]')
    if mel_len is not None:
        _chk(mel_len, 'mel_len', torch.int64)
    out = alloc(B * (Tmax + tail), cout, dtype=torch.float32, device=mel.device)
    extra = (tail, float(pad_value)) if family == 'melgan' else ()      # (HiFi-GAN's entry points take no tail)
    _lib.call(f'ft_{family}_conv_in', _p(mel), _p(mel_len), B, C, Tmax, *extra, _p(w), _p(bias), cout, _p(out), _p(err),
              _stream())
    return out


def _voc_upsample(family, x, mel_len, B, Tmax, tail, scale, stride, w, bias, cout, alloc):
    _chk(x, 'x'); _chk(w, 'w'); _chk(bias, 'bias')
    rows, cin = x.shape
    CP = -(-cout // 32) * 32
    if rows != B * (Tmax + tail) * scale or tuple(w.shape) != (2 * stride, cin, CP) or bias.numel() != CP:
        raise _lib.FtError(f'{family}_upsample: x {tuple(x.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)} for '
                           f'{B * (Tmax + tail) * scale} rows and w [{2 * stride}, {cin}, {CP}]')
    out = alloc(rows * stride, cout, dtype=torch.float32, device=x.device)
    extra = (tail,) if family == 'melgan' else ()
    _lib.call(f'ft_{family}_upsample', _p(x), _p(mel_len), B, Tmax, *extra, scale, cin, cout, stride, _p(w), _p(bias),
              _p(out), _stream())
    return out


def _voc_conv_out(family, x, mel_len, B, Tmax, tail, scale, w, bias, alloc):
    _chk(x, 'x'); _chk(w, 'w')
    rows, C = x.shape
    if rows != B * (Tmax + tail) * scale or tuple(w.shape) != (C, 32):
        raise _lib.FtError(f'{family}_conv_out: x {tuple(x.shape)}, w {tuple(w.shape)} for {B * (Tmax + tail) * scale} rows '
                           f'and w [{C}, 32]')
    wav = alloc(B, Tmax * scale, dtype=torch.float32, device=x.device)
    i16 = alloc(B, Tmax * scale, dtype=torch.int16, device=x.device)
    extra = (tail,) if family == 'melgan' else ()
    _lib.call(f'ft_{family}_conv_out', _p(x), _p(mel_len), B, Tmax, *extra, scale, C, _p(w), float(bias), _p(wav), _p(i16),
              _stream())
    return wav, i16


def melgan_conv_in(mel: torch.Tensor, mel_len: Optional[torch.Tensor], tail: int, pad_value: float, w: torch.Tensor,
                   bias: torch.Tensor, cout: int, err: Optional[torch.Tensor] = None, alloc=torch.empty) -> torch.Tensor:
    """mel [B, n_mels, Tmax] -> [B * (Tmax + tail), cout]: normalise, append the tail, reflect 3, Conv1d(k = 7)"""
    return _voc_conv_in('melgan', mel, mel_len, tail, pad_value, w, bias, cout, err, alloc)


def melgan_upsample(x: torch.Tensor, mel_len: Optional[torch.Tensor], B: int, Tmax: int, tail: int, scale: int,
                    stride: int, w: torch.Tensor, bias: torch.Tensor, cout: int, alloc=torch.empty) -> torch.Tensor:
    """x [B * (Tmax + tail) * scale, cin] -> [B * (Tmax + tail) * scale * stride, cout]: LeakyReLU + ConvTranspose1d"""
    return _voc_upsample('melgan', x, mel_len, B, Tmax, tail, scale, stride, w, bias, cout, alloc)


def melgan_conv_out(x: torch.Tensor, mel_len: Optional[torch.Tensor], B: int, Tmax: int, tail: int, scale: int,
                    w: torch.Tensor, bias: float, alloc=torch.empty):
    """x [B * (Tmax + tail) * scale, C] -> (wav float32 [B, Tmax * scale], zero at j >= mel_len[b] * scale; wav_int16)"""
    return _voc_conv_out('melgan', x, mel_len, B, Tmax, tail, scale, w, bias, alloc)


def hifigan_conv_in(mel: torch.Tensor, mel_len: Optional[torch.Tensor], w: torch.Tensor, bias: torch.Tensor, cout: int,
                    err: Optional[torch.Tensor] = None, alloc=torch.empty) -> torch.Tensor:
    """mel [B, n_mels, Tmax] -> [B * Tmax, cout]: Conv1d(k = 7, padding 3) of the mel as it is"""
    return _voc_conv_in('hifigan', mel, mel_len, 0, 0.0, w, bias, cout, err, alloc)


def hifigan_upsample(x: torch.Tensor, mel_len: Optional[torch.Tensor], B: int, Tmax: int, scale: int, stride: int,
                     w: torch.Tensor, bias: torch.Tensor, cout: int, alloc=torch.empty) -> torch.Tensor:
    """x [B * Tmax * scale, cin] -> [B * Tmax * scale * stride, cout]: LeakyReLU(0.1) + ConvTranspose1d"""
    return _voc_upsample('hifigan', x, mel_len, B, Tmax, 0, scale, stride, w, bias, cout, alloc)


def hifigan_conv_out(x: torch.Tensor, mel_len: Optional[torch.Tensor], B: int, Tmax: int, scale: int, w: torch.Tensor,
                     bias: float, alloc=torch.empty):
    """x [B * Tmax * scale, C] -> (wav float32 [B, Tmax * scale], zero at j >= mel_len[b] * scale; wav_int16)"""
    return _voc_conv_out('hifigan', x, mel_len, B, Tmax, 0, scale, w, bias, alloc)


def melgan_resblock(x: torch.Tensor, mel_len: Optional[torch.Tensor], B: int, Tmax: int, tail: int, scale: int,
                    dilation: int, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                    ws: torch.Tensor, bs: torch.Tensor, out: Optional[torch.Tensor] = None, alloc=torch.empty
                    ) -> torch.Tensor:
    """x [B * (Tmax + tail) * scale, C] -> the residual block at `dilation`, one launch (out: a buffer of x's shape)"""
    for t in (x, w1, b1, w2, b2, ws, bs):
        _chk(t, 'melgan_resblock operand')
    rows, C = x.shape
    CP = -(-C // 32) * 32
    if rows != B * (Tmax + tail) * scale or tuple(w1.shape) != (3, C, CP) or tuple(w2.shape) != (C, CP) or \
            tuple(ws.shape) != (C, CP) or any(b.numel() != CP for b in (b1, b2, bs)):
        raise _lib.FtError(f'melgan_resblock: x {tuple(x.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}, ws '
                           f'{tuple(ws.shape)} for {B * (Tmax + tail) * scale} rows and [{C}, {CP}] panels')
    if out is None:
        out = alloc(rows, C, dtype=torch.float32, device=x.device)
    elif _chk(out, 'out').shape != x.shape or out.data_ptr() == x.data_ptr():
        raise _lib.FtError('melgan_resblock: out must be another buffer of the shape of x')
    _lib.call('ft_melgan_resblock', _p(x), _p(mel_len), B, Tmax, tail, scale, C, dilation, _p(w1), _p(b1), _p(w2), _p(b2),
              _p(ws), _p(bs), _p(out), _stream())
    return out


def _hifigan_out(what: str, x: torch.Tensor, out: Optional[torch.Tensor], acc_mode: int, alloc) -> torch.Tensor:
    if acc_mode not in (0, 1, 2):
        raise _lib.FtError(f'{what}: acc_mode {acc_mode} (0 store, 1 add, 2 add and divide by nk)')
    if out is None:
        if acc_mode:
            raise _lib.FtError(f'{what}: accumulating needs the buffer that holds the sum')
        return alloc(*x.shape, dtype=torch.float32, device=x.device)
    if _chk(out, 'out').shape != x.shape or out.data_ptr() == x.data_ptr():
        raise _lib.FtError(f'{what}: out must be another buffer of the shape of x')
    return out


def hifigan_resconv(x: torch.Tensor, mel_len: Optional[torch.Tensor], B: int, Tmax: int, scale: int, dilation: int,
                    w: torch.Tensor, bias: torch.Tensor, res: Union[None, str, torch.Tensor] = None, acc_mode: int = 0,
                    nk: int = 1, out: Optional[torch.Tensor] = None, alloc=torch.empty) -> torch.Tensor:
    """x [B * Tmax * scale, C] -> res + bias + Conv1d(k, dilation, zero padding)(lrelu_0.1(x)); w [k, C, CP].  res: None,
    'x' (the input itself) or another [rows, C] buffer.  acc_mode 0: out = value, 1: out += value, 2: out = (out +
    value) / nk."""
    _chk(x, 'x'); _chk(w, 'w'); _chk(bias, 'bias')
    rows, C = x.shape
    CP = -(-C // 32) * 32
    if rows != B * Tmax * scale or w.dim() != 3 or tuple(w.shape[1:]) != (C, CP) or bias.numel() != CP:
        raise _lib.FtError(f'hifigan_resconv: x {tuple(x.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)} for '
                           f'{B * Tmax * scale} rows and w [k, {C}, {CP}]')
    res_mode = 0 if res is None else 1 if isinstance(res, str) and res == 'x' else 2
    if res_mode == 2 and (not isinstance(res, torch.Tensor) or _chk(res, 'res').shape != x.shape):
        raise _lib.FtError("hifigan_resconv: res must be None, 'x' or a buffer of the shape of x")
    out = _hifigan_out('hifigan_resconv', x, out, acc_mode, alloc)
    _lib.call('ft_hifigan_resconv', _p(x), _p(mel_len), B, Tmax, scale, C, int(w.shape[0]), dilation, _p(w), _p(bias),
              _p(res) if res_mode == 2 else None, res_mode, acc_mode, nk, _p(out), _stream())
    return out


def hifigan_respair(x: torch.Tensor, mel_len: Optional[torch.Tensor], B: int, Tmax: int, scale: int, dilation: int,
                    w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, acc_mode: int = 0, nk: int = 1,
                    out: Optional[torch.Tensor] = None, alloc=torch.empty) -> torch.Tensor:
    """ResBlock1's pair in one launch: x + b2 + Conv1d(k)(lrelu(b1 + Conv1d(k, dilation)(lrelu(x)))); w1, w2 [k, C, CP]"""
    for t in (x, w1, b1, w2, b2):
        _chk(t, 'hifigan_respair operand')
    rows, C = x.shape
    CP = -(-C // 32) * 32
    if rows != B * Tmax * scale or w1.dim() != 3 or tuple(w1.shape[1:]) != (C, CP) or w2.shape != w1.shape or \
            b1.numel() != CP or b2.numel() != CP:
        raise _lib.FtError(f'hifigan_respair: x {tuple(x.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)} for '
                           f'{B * Tmax * scale} rows and [k, {C}, {CP}] panels')
    out = _hifigan_out('hifigan_respair', x, out, acc_mode, alloc)
    _lib.call('ft_hifigan_respair', _p(x), _p(mel_len), B, Tmax, scale, C, int(w1.shape[0]), dilation, _p(w1), _p(b1),
              _p(w2), _p(b2), acc_mode, nk, _p(out), _stream())
    return out


_H16_FIELDS = ('tile_rows', 'lds_bytes', 'threads', 'staged', 'cpad')


def hifigan_h16_plan(field: str, c: int) -> int:
    """the launch plan of the fp16-operand residual convolution for width c (csrc/ft_voc_plan_h16.h): field 'tile_rows',
    'lds_bytes' (static LDS of the workgroup), 'threads', 'staged' (the widest width the arrangement stages) or 'cpad' (c
    rounded up to the 16 the MFMA contracts at a time); 0 where the width is not supported"""
    return int(_lib.query('ft_hifigan_h16_plan', _H16_FIELDS.index(field), int(c)))


def hifigan_resconv_h16(x: torch.Tensor, mel_len: Optional[torch.Tensor], B: int, Tmax: int, scale: int, dilation: int,
                        w: torch.Tensor, bias: torch.Tensor, res: Union[None, str, torch.Tensor] = None, acc_mode: int = 0,
                        nk: int = 1, out: Optional[torch.Tensor] = None, alloc=torch.empty) -> torch.Tensor:
    """hifigan_resconv with fp16 matrix operands (HiFiGAN.matmul_dtype = 'fp16'): x [B * Tmax * scale, C] fp32 -> res + bias
    + Conv1d(k, dilation, zero padding)(fp16(clamp(lrelu_0.1(x)))) accumulated in fp32; w: the fp16 pack of
    hifigan.pack_taps_h16, [k, cpad / 8, CP, 8]; bias, res, acc_mode, nk and out as in hifigan_resconv."""
    _chk(x, 'x'); _chk(w, 'w', torch.float16); _chk(bias, 'bias')
    rows, C = x.shape
    CP = -(-C // 32) * 32
    cpad = -(-C // 16) * 16
    if rows != B * Tmax * scale or w.dim() != 4 or tuple(w.shape[1:]) != (cpad // 8, CP, 8) or bias.numel() != CP:
        raise _lib.FtError(f'hifigan_resconv_h16: x {tuple(x.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)} for '
                           f'{B * Tmax * scale} rows and w [k, {cpad // 8}, {CP}, 8]')
    res_mode = 0 if res is None else 1 if isinstance(res, str) and res == 'x' else 2
    if res_mode == 2 and (not isinstance(res, torch.Tensor) or _chk(res, 'res').shape != x.shape):
        raise _lib.FtError("hifigan_resconv_h16: res must be None, 'x' or a buffer of the shape of x")
    out = _hifigan_out('hifigan_resconv_h16', x, out, acc_mode, alloc)
    _lib.call('ft_hifigan_resconv_h16', _p(x), _p(mel_len), B, Tmax, scale, C, int(w.shape[0]), dilation, _p(w), _p(bias),
              _p(res) if res_mode == 2 else None, res_mode, acc_mode, nk, _p(out), _stream())
    return out
