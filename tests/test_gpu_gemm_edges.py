"""GPU: the 128-tile GEMM kernels at ragged edges, each case pinned to the kernel it means to exercise.

tests/test_gpu_primitives.py checks the GEMM-shaped entry points at small odd shapes (the 64x64 f32 kernels) and at large
ROUND shapes (the 128x128 bf16-split kernels).  This file covers what lies between: shapes just past the launcher's
128-tile threshold (gemm_plan::tiles_big: 192 tiles -- 12,300 rows x 130..200 columns give 194) whose M, N and K are no
multiples of the tile or of the 16-deep stage.  Every case

  * asserts the launch-variant counter delta (hip.gemm_variant_counts) of the ONE kernel it is about -- a planner
    threshold that moves the shape onto another kernel fails the case instead of quietly testing less;
  * compares with a float64 CPU product at the project's existing bars: rel_err < 2e-6 (test_linear_fwd_bwd), the
    element-wise |got - ref| / (|A| |B| + |bias|) < 1e-6 of test_large_gemm_split_path_is_fp32_accurate where the operands
    get that test's wide dynamic range, and for the bf16 mode the reference and bar of
    test_bf16_gemm_rounds_operands_and_accumulates_in_fp32;
  * poisons the surroundings: operands are carved from NaN-filled buffers (NaN in the row padding between the row length
    and the leading dimension where the entry point takes one), the output is a column slice of a wider NaN-filled buffer
    with NaN guard rows; the result must be finite and every guard element still NaN.  A tail that reads one element too
    many or stores one too far shows up instead of cancelling.
"""
import ctypes

import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

NAN = float('nan')


@pytest.fixture(scope='module')
def H():
    from forwardtacotron_amd import hip
    assert torch.cuda.is_available()
    return hip


def _call(name, *args):
    from forwardtacotron_amd import _lib
    _lib.call(name, *args)


def elem_err(got, ref, scale):
    return float(((got - ref).abs() / (scale + 1e-30)).max())


def gen(seed):
    return torch.Generator().manual_seed(seed)


def wide(g, rows, cols, spread):
    """full-mantissa values whose rows span a wide dynamic range (as test_large_gemm_split_path_is_fp32_accurate)"""
    return torch.randn(rows, cols, generator=g) * torch.exp(spread * torch.randn(rows, 1, generator=g))


def poison(t, ld=None, mis=0):
    """Device copy of the matrix t [R, C] with row stride ld inside a NaN-filled buffer: NaN between C and ld and eight
    rows' worth of NaN in front and behind.  mis = floats by which the base misses 16-byte alignment.  The view keeps the
    buffer alive; view.data_ptr() is the operand's address."""
    t = t.reshape(t.shape[0], -1)
    R, C = t.shape
    ld = ld or C
    front = 8 * ld + (-8 * ld) % 4 + mis
    buf = torch.full((front + R * ld + 8 * ld,), NAN, device='cuda')
    view = buf[front:front + R * ld].view(R, ld)[:, :C]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * mis
    return view


class Out:
    """[rows, cols] output as a column slice (unaligned: 5 columns in, row stride cols + 9) of a NaN-filled buffer with three
    guard rows above and below; flat = contiguous (entry points without a leading dimension: guard rows only)."""

    def __init__(self, rows, cols, prior=None, flat=False):
        self.rows, self.cols = rows, cols
        self.ld, self.c0 = (cols, 0) if flat else (cols + 9, 5)
        self.buf = torch.full((rows + 6, self.ld), NAN, device='cuda')
        self.view = self.buf[3:3 + rows, self.c0:self.c0 + cols]
        if prior is not None:
            self.view.copy_(prior)
        self.ptr = self.view.data_ptr()

    def check(self):
        got = self.view.cpu()
        g = self.buf.clone()
        g[3:3 + self.rows, self.c0:self.c0 + self.cols] = NAN
        assert bool(torch.isnan(g).all()), 'a guard element around the output was overwritten'
        bad = (~torch.isfinite(got)).nonzero()
        assert bad.numel() == 0, f'{bad.shape[0]} non-finite outputs, first at {bad[0].tolist()}'
        return got.double()


def counted(H, want, fn):
    """run fn; the GEMM launches it made must be exactly `want` ({variant: launches} or one variant name)"""
    if isinstance(want, str):
        want = {want: 1}
    before = H.gemm_variant_counts()
    fn()
    after = H.gemm_variant_counts()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert delta == want, f'kernel choice drifted: launched {delta}, this case is about {want}'


def ptr(t):
    return None if t is None else t.data_ptr()


def linear_fwd(H, x, ldx, w, b, out, M, K, N, relu=0, acc=0, x_tm=0, y_tm=0):
    _call('ft_linear_fwd', ptr(x), ldx, ptr(w), ptr(b), out.ptr, out.ld, M, K, N, relu, acc, x_tm, y_tm, H._stream())


# ---------------------------------------------------------------------------------------------------
# NT, pipelined 128x128 kernel: K tails of the 16-deep stage (K % 16 in {4, 8, 12}, K < 16, none), M % 128 = 12 and an N
# tail in the second column tile; bias / ReLU / accumulate epilogues
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [200, 130])
@pytest.mark.parametrize('K', [12, 16, 36, 40, 44, 260])
def test_nt_pipelined_k_tails(H, N, K):
    M = 12300
    g = gen(1000 * K + N)
    x = wide(g, M, K, 3.0)
    w = wide(g, N, K, 1.0)
    b = torch.randn(N, generator=g)
    prior = wide(g, M, N, 3.0)
    ldx = K + 12
    xd, wd, bd = poison(x, ldx), poison(w), poison(b[None])
    ref = x.double() @ w.double().t()
    scale = x.double().abs() @ w.double().abs().t()
    for bias, relu, acc in ((0, 0, 0), (1, 1, 0), (1, 0, 1)):
        out = Out(M, N, prior if acc else None)
        counted(H, 'rows_b3p', lambda: linear_fwd(H, xd, ldx, wd, bd if bias else None, out, M, K, N, relu, acc))
        got = out.check()
        r, s = ref, scale
        if bias:
            r, s = r + b.double(), s + b.double().abs()
        if relu:
            r = r.clamp_min(0)
        if acc:
            r, s = r + prior.double(), s + prior.double().abs()
        e = elem_err(got, r, s)
        assert e < 1e-6, (bias, relu, acc, e)


# ---------------------------------------------------------------------------------------------------
# NT, pipelined kernel: convolution taps x K tail (Cin = 36: the tail mask is re-armed on every tap; rows leave the time
# window at both ends of every item; 24 x 513 rows: tiles straddle items)
# ---------------------------------------------------------------------------------------------------
def _conv_case(k, seed):
    B, T, Cin, Cout = 24, 513, 36, 200
    Tout = T if k % 2 else T + 1
    g = gen(seed)
    x = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, generator=g)
    xp = torch.nn.functional.pad(x.double(), (0, 0, k // 2, k // 2))
    ref = sum(xp[:, j:j + Tout] @ w[:, :, j].double().t() for j in range(k)).reshape(B * Tout, Cout)
    return B, T, Cin, Cout, Tout, g, x, w, ref


@pytest.mark.parametrize('k', [5, 4])
def test_nt_pipelined_conv_taps_with_k_tail(H, k):
    B, T, Cin, Cout, Tout, g, x, w, ref = _conv_case(k, 50 + k)
    M = B * Tout
    ldx = Cin + 4
    xd = poison(x.reshape(B * T, Cin), ldx)
    wp = poison(w.permute(2, 0, 1).reshape(k * Cout, Cin))                 # tap-major [k][Cout][Cin]
    sc = torch.rand(Cout, generator=g) + 0.5
    sh = torch.randn(Cout, generator=g)
    bias = torch.randn(Cout, generator=g)
    prior = torch.randn(M, Cout, generator=g)
    scd, shd, bd = poison(sc[None]), poison(sh[None]), poison(bias[None])

    def conv(out, scale, shift, relu, acc):
        _call('ft_conv1d_fwd', ptr(xd), ldx, ptr(wp), ptr(scale), ptr(shift), out.ptr, out.ld, B, T, Cin, Cout, k, Tout,
              relu, acc, H._stream())

    out = Out(M, Cout)
    counted(H, 'rows_b3p', lambda: conv(out, None, None, 0, 0))
    assert rel_err(out.check(), ref) < 2e-6
    out = Out(M, Cout)                                                   # eval-mode BatchNorm fold: relu, then scale / shift
    counted(H, 'rows_b3p', lambda: conv(out, scd, shd, 1, 0))
    assert rel_err(out.check(), ref.clamp_min(0) * sc.double() + sh.double()) < 2e-6
    out = Out(M, Cout, prior)
    counted(H, 'rows_b3p', lambda: conv(out, None, None, 0, 1))
    assert rel_err(out.check(), ref + prior.double()) < 2e-6
    if k % 2:
        out = Out(M, Cout)
        counted(H, 'rows_b3p', lambda: _call('ft_conv1d_bias_fwd', ptr(xd), ldx, ptr(wp), ptr(bd), out.ptr, out.ld, B, T,
                                             Cin, Cout, k, 1, H._stream()))
        assert rel_err(out.check(), (ref + bias.double()).clamp_min(0)) < 2e-6


@pytest.mark.parametrize('k,masked', [(5, True), (4, False)])
def test_nt_pipelined_conv_data_gradient(H, k, masked):
    """dx = sum over taps of shifted dy * W (contraction over Cout = 36: K tail on every tap, DEscending row shifts);
    masked: through the ReLU-mask epilogue (ft_conv1d_bwd_data_relu), else ft_conv1d_bwd_data on a [B, T+1] gradient"""
    B, T, Cin, Cout = 24, 513, 200, 36
    Tbuf = T if masked else T + 1
    g = gen(70 + k)
    dy = torch.randn(B, Tbuf, Cout, generator=g)
    w = torch.randn(Cout, Cin, k, generator=g)
    p = k // 2
    dyp = torch.nn.functional.pad(dy.double(), (0, 0, p, p))
    ref = sum(dyp[:, 2 * p - j:2 * p - j + T] @ w[:, :, j].double() for j in range(k)).reshape(B * T, Cin)
    lddy = Cout + 8
    dyd = poison(dy.reshape(B * Tbuf, Cout), lddy)
    wpt = poison(w.permute(2, 1, 0).reshape(k * Cin, Cout))              # transposed tap-major [k][Cin][Cout]
    out = Out(B * T, Cin)
    if masked:
        y = torch.randn(B * T, Cin, generator=g)
        ymask = Out(B * T, Cin, y)                                        # the mask is read at the output's own indices
        counted(H, 'rows_b3p', lambda: _call('ft_conv1d_bwd_data_relu', ptr(dyd), lddy, ptr(wpt), ymask.ptr, out.ptr,
                                             out.ld, B, T, Cin, Cout, k, 1, H._stream()))
        ref = ref * (y > 0).double()
    else:
        counted(H, 'rows_b3p', lambda: _call('ft_conv1d_bwd_data', ptr(dyd), lddy, ptr(wpt), out.ptr, out.ld, B, T, Cin,
                                             Cout, k, Tbuf, Tbuf, 0, 1, H._stream()))
    assert rel_err(out.check(), ref) < 2e-6


# ---------------------------------------------------------------------------------------------------
# NT, pipelined kernel: time-major row maps.  B = 24 does not divide 128 and T = 513 is no multiple of it, so 128-row
# tiles straddle batch items (the row0 selection of the kernel's setup) on the input side, the output side, and both
# ---------------------------------------------------------------------------------------------------
def _tm_case(seed, spread):
    B, T, K, N = 24, 513, 36, 200
    g = gen(seed)
    x = wide(g, B * T, K, spread)
    w = wide(g, N, K, 1.0 if spread else 0.0)
    b = torch.randn(N, generator=g)
    return B, T, K, N, x, w, b


def _to_tm(t, B, T):
    """[B*T, C] batch-major rows -> the same rows stored time-major"""
    return t.view(B, T, -1).transpose(0, 1).reshape(T * B, -1)


@pytest.mark.parametrize('x_tm,y_tm', [(1, 0), (0, 1), (1, 1)])
def test_nt_pipelined_time_major_maps(H, x_tm, y_tm):
    B, T, K, N, x, w, b = _tm_case(90 + 2 * x_tm + y_tm, 3.0)
    M = B * T
    ldx = K + 4
    xd = poison(_to_tm(x, B, T) if x_tm else x, ldx)
    wd, bd = poison(w), poison(b[None])
    out = Out(M, N)
    counted(H, 'rows_b3p', lambda: linear_fwd(H, xd, ldx, wd, bd, out, M, K, N, 0, 0, B * x_tm, B * y_tm))
    got = out.check()
    ref = x.double() @ w.double().t() + b.double()
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    if y_tm:
        ref, scale = _to_tm(ref, B, T), _to_tm(scale, B, T)
    assert elem_err(got, ref, scale) < 1e-6


# ---------------------------------------------------------------------------------------------------
# bf16 precision mode of the same launches (one bf16 plane: another LDS row stride); reference and bar of
# test_bf16_gemm_rounds_operands_and_accumulates_in_fp32
# ---------------------------------------------------------------------------------------------------
def _bf16_check(got, x, w, b, K):
    ref = x.bfloat16().double() @ w.bfloat16().double().t() + b.double()
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err < 2e-6 * scale * max(1.0, (K / 64) ** 0.5), (K, err / scale)
    return ref


@pytest.mark.parametrize('K', [12, 44, 260])
def test_nt_pipelined_k_tails_bf16_mode(H, K):
    M, N = 12300, 130
    g = gen(300 + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g)
    ldx = K + 12
    xd, wd, bd = poison(x, ldx), poison(w), poison(b[None])
    out = Out(M, N)
    old = H.set_gemm_precision('bf16')
    try:
        counted(H, 'rows_b3p', lambda: linear_fwd(H, xd, ldx, wd, bd, out, M, K, N))
    finally:
        H.set_gemm_precision(old)
    got = out.check()
    ref = _bf16_check(got, x, w, b, K)
    scale = float(ref.abs().max())
    err = float((got - (x.double() @ w.double().t() + b.double())).abs().max())
    assert 1e-4 * scale < err < 3e-2 * scale, (K, err / scale)          # genuinely bf16 operands, not fp32


@pytest.mark.parametrize('x_tm,y_tm', [(1, 0), (0, 1), (1, 1)])
def test_nt_pipelined_time_major_maps_bf16_mode(H, x_tm, y_tm):
    B, T, K, N, x, w, b = _tm_case(190 + 2 * x_tm + y_tm, 0.0)
    M = B * T
    ldx = K + 4
    xd = poison(_to_tm(x, B, T) if x_tm else x, ldx)
    wd, bd = poison(w), poison(b[None])
    out = Out(M, N)
    old = H.set_gemm_precision('bf16')
    try:
        counted(H, 'rows_b3p', lambda: linear_fwd(H, xd, ldx, wd, bd, out, M, K, N, 0, 0, B * x_tm, B * y_tm))
    finally:
        H.set_gemm_precision(old)
    got = out.check()
    if y_tm:
        got = got.view(T, B, N).transpose(0, 1).reshape(M, N)
    _bf16_check(got, x, w, b, K)


def test_bf16_mode_small_shapes_take_the_64_tile_split_kernels(H):
    """below the 128-tile threshold the bf16 mode runs the one-plane 64x64 kernels (NT and TN), ragged in every dimension
    the 16-byte-load path allows"""
    M, N, K = 333, 132, 36
    g = gen(7)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    xd, wd, bd, dyd = poison(x, K + 4), poison(w), poison(b[None]), poison(dy, N + 4)
    out = Out(M, N)
    dw = Out(N, K, flat=True)
    ws = H.workspace(H._lib.query('ft_linear_bwd_weight_workspace', M, K, N), 'cuda')
    old = H.set_gemm_precision('bf16')
    try:
        counted(H, 'rows_b3_64', lambda: linear_fwd(H, xd, K + 4, wd, bd, out, M, K, N))
        counted(H, 'tn_b3_64', lambda: _call('ft_linear_bwd_weight', ptr(dyd), N + 4, ptr(xd), K + 4, dw.ptr, M, K, N, 1, M,
                                             0, 0, 0, 0, ptr(ws), ws.numel(), H._stream()))
    finally:
        H.set_gemm_precision(old)
    _bf16_check(out.check(), x, w, b, K)
    _bf16_check(dw.check(), dy.t().contiguous(), x.t().contiguous(), torch.zeros(K), M)


# ---------------------------------------------------------------------------------------------------
# the 128-tile kernels behind the split path: f32 MFMA, not fast (scalar loads) and the NN form
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,K,mis', [(200, 37, 0), (130, 37, 0), (200, 36, 1)])
def test_big_tile_f32_fallback_nt(H, N, K, mis):
    """K % 4 != 0, or an operand base that misses 16-byte alignment by one float: no 16-byte loads, so the launch stays
    on the f32 128x128 kernel's scalar-load form"""
    M = 12300
    g = gen(400 + N + K + mis)
    x = wide(g, M, K, 3.0)
    w = wide(g, N, K, 1.0)
    b = torch.randn(N, generator=g)
    ldx = 44
    xd, wd, bd = poison(x, ldx, mis), poison(w), poison(b[None])
    ref = x.double() @ w.double().t() + b.double()
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    for relu in (0, 1):
        out = Out(M, N)
        counted(H, 'rows_f32_128_nt_slow', lambda: linear_fwd(H, xd, ldx, wd, bd, out, M, K, N, relu))
        assert elem_err(out.check(), ref.clamp_min(0) if relu else ref, scale) < 1e-6, relu


@pytest.mark.parametrize('K,form', [(37, 'plain'), (36, 'plain'), (37, 'rowpad')])
def test_big_tile_f32_nn(H, K, form):
    """C = A [M, K] * B [K, N] with B's N contiguous (data gradient through an untransposed weight; attention's P V):
    K % 4 != 0 takes the scalar-load form unless the caller declares A's rows padded (ft_bgemm_nn's a_rows_padded: the
    padding is NaN here -- the kernel must not let it reach a sum)"""
    M, N = 12300, 200
    g = gen(500 + K + len(form))
    a = wide(g, M, K, 3.0)
    bm = torch.randn(K, N, generator=g)
    lda = (K + 3) // 4 * 4 if form == 'rowpad' else K + 4
    ad, bmd = poison(a, lda), poison(bm)
    ref = a.double() @ bm.double()
    scale = a.double().abs() @ bm.double().abs()
    out = Out(M, N)
    if form == 'rowpad':
        counted(H, 'rows_f32_128_nn_fast', lambda: _call('ft_bgemm_nn', ptr(ad), lda, 0, 0, ptr(bmd), N, 0, 0, out.ptr,
                                                         out.ld, 0, 0, M, N, K, 1, 1, 1, H._stream()))
    else:                                                                 # w [out_f = K][in_f = N], w_transposed = 0
        counted(H, 'rows_f32_128_nn_fast' if K % 4 == 0 else 'rows_f32_128_nn_slow',
                lambda: _call('ft_linear_bwd_data', ptr(ad), lda, ptr(bmd), out.ptr, out.ld, M, N, K, 0, 0, 0, 0,
                              H._stream()))
    assert elem_err(out.check(), ref, scale) < 1e-6


def test_two_barrier_nt_kernel_behind_a_long_row_stride(H):
    """The pipelined kernel addresses a tile's rows with 31-bit byte offsets; a row stride that takes a tile's span past
    2 GiB (here: time-major rows 34,900 floats apart) leaves the launch on the two-barrier 128x128 kernel, which walks
    64-bit pointers.  Same ragged M / N / K and straddling tiles as the time-major cases above."""
    B, T, K, N, x, w, b = _tm_case(600, 3.0)
    M = B * T
    ldx = 34900
    xd = poison(_to_tm(x, B, T), ldx)
    wd, bd = poison(w), poison(b[None])
    out = Out(M, N)
    counted(H, 'rows_b3_128', lambda: linear_fwd(H, xd, ldx, wd, bd, out, M, K, N, 0, 0, B, 0))
    ref = x.double() @ w.double().t() + b.double()
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    assert elem_err(out.check(), ref, scale) < 1e-6


# ---------------------------------------------------------------------------------------------------
# split-K of NT launches (gemm_plan::rows_ksplit, ft_ksplit_reduce_kernel)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,tmB', [(200, 0), (200, 8), (4096, 0), (4096, 32)])
@pytest.mark.parametrize('acc', [0, 1])
def test_split_k_of_a_chained_data_gradient(H, rows, tmB, acc):
    """dx (+)= dy_0 W_0 + dy_1 W_1 with out_f = 2052 each: 2 x 129 stages cut into 8 ranges of 33 -- range 3 crosses the
    task boundary, the ranges that end a task carry its K tail of 4 -- reduced with accumulate and (tmB) a time-major
    output map.  The same call without scratch takes the unsplit kernel; both are compared with float64 only (they sum
    in different orders by design)."""
    in_f, out_f, nt = 132, 2052, 2
    g = gen(700 + rows + tmB)
    dys = [wide(g, rows, out_f, 2.0) for _ in range(nt)]
    wts = [torch.randn(in_f, out_f, generator=g) for _ in range(nt)]     # W^T [in_f][out_f]: w_transposed = 1
    prior = torch.randn(rows, in_f, generator=g)
    lddy = out_f + 4
    dyd = [poison(d, lddy) for d in dys]
    wd = [poison(w) for w in wts]
    ref = sum(d.double() @ w.double().t() for d, w in zip(dys, wts))
    scale = sum(d.double().abs() @ w.double().abs().t() for d, w in zip(dys, wts))
    if acc:
        ref, scale = ref + prior.double(), scale + prior.double().abs()
    if tmB:
        ref, scale, prior = (_to_tm(t, tmB, rows // tmB) for t in (ref, scale, prior))
    da = (ctypes.c_void_p * nt)(*[d.data_ptr() for d in dyd])
    wa = (ctypes.c_void_p * nt)(*[w.data_ptr() for w in wd])
    nbytes = H._lib.lib().ft_linear_bwd_data_multi_workspace(nt, rows, in_f, out_f, H._stream())
    assert nbytes > 0, 'the planner no longer splits this shape'
    ws = torch.full((nbytes // 4 + 64,), NAN, device='cuda')

    def run(out, scratch):
        _call('ft_linear_bwd_data_multi_ws', nt, ctypes.cast(da, ctypes.c_void_p), lddy, ctypes.cast(wa, ctypes.c_void_p),
              out.ptr, out.ld, rows, in_f, out_f, acc, 0, tmB, 1, ptr(scratch), nbytes if scratch is not None else 0,
              H._stream())

    out = Out(rows, in_f, prior if acc else None)
    counted(H, 'rows_b3p_ksplit', lambda: run(out, ws))
    assert elem_err(out.check(), ref, scale) < 1e-6
    assert bool(torch.isnan(ws[nbytes // 4:]).all()), 'the split wrote past the scratch size the query asked for'
    out = Out(rows, in_f, prior if acc else None)
    counted(H, 'rows_f32_64_nt_fast', lambda: run(out, None))            # no scratch: one pass over K (64 tiles or fewer)
    assert elem_err(out.check(), ref, scale) < 1e-6


@pytest.mark.parametrize('C,variant', [(100, 'rows_b3p_ksplit'), (132, 'rows_b3p')])
def test_split_k_of_the_conv_bank_data_gradient(H, C, variant):
    """ft_conv_bank_bwd_data with few output tiles (its workspace query answers non-zero): K = 8 members of 1..8 taps, a K
    tail of 4 on every tap.  C = 100: 252 stages chained into one product and cut into 7 ranges that start inside members
    and taps -- split-K, whose 7 partial slabs fit the K slabs the query asks for.  C = 132: 324 stages would be cut into 10
    ranges, more than that scratch holds, so the members run as K tasks of one launch into their own slabs and an ordered
    sum follows."""
    B, T, Cin, K = 9, 171, 132, 8
    Tbuf = T + 1
    g = gen(800)
    dy = torch.randn(B, Tbuf, K * C, generator=g)
    wk = [torch.randn(C, Cin, k, generator=g) for k in range(1, K + 1)]
    ref = torch.zeros(B, T, Cin, dtype=torch.float64)
    for i, w in enumerate(wk):
        k, p = i + 1, (i + 1) // 2
        d = dy[:, :, i * C:(i + 1) * C].double().clone()
        if k % 2:
            d[:, T:] = 0                                                  # an odd member's output has T rows
        dp = torch.nn.functional.pad(d, (0, 0, p, k))
        for j in range(k):
            ref += dp[:, 2 * p - j:2 * p - j + T] @ w[:, :, j].double()
    ref = ref.reshape(B * T, Cin)
    lddy = K * C + 4
    dyd = poison(dy.reshape(B * Tbuf, K * C), lddy)
    wpt = poison(torch.cat([w.permute(2, 1, 0).reshape(-1) for w in wk])[None])
    nbytes = H._lib.query('ft_conv_bank_bwd_data_workspace', B, T, Cin, K)
    assert nbytes > 0, 'the planner no longer splits this shape'
    ws = torch.full((nbytes // 4 + 64,), NAN, device='cuda')
    out = Out(B * T, Cin)
    counted(H, variant, lambda: _call('ft_conv_bank_bwd_data', ptr(dyd), lddy, ptr(wpt), out.ptr, out.ld, B, T, Cin, C, K,
                                      Tbuf, 1, ptr(ws), nbytes, H._stream()))
    assert rel_err(out.check(), ref) < 2e-6
    assert bool(torch.isnan(ws[nbytes // 4:]).all())


# ---------------------------------------------------------------------------------------------------
# TN (weight gradients), 128x128 tile: M / N tails in the slab and reduce addressing, ragged contraction rows
# ---------------------------------------------------------------------------------------------------
def _wgrad(H, dyd, lddy, xd, ldx, dw, rows, in_f, out_f, B=1, T=0, shift=0, acc=0, dy_tm=0, x_tm=0):
    ws = H.workspace(H._lib.query('ft_linear_bwd_weight_workspace', rows, in_f, out_f), 'cuda')
    _call('ft_linear_bwd_weight', ptr(dyd), lddy, ptr(xd), ldx, dw.ptr, rows, in_f, out_f, B, T or rows, shift, acc, dy_tm,
          x_tm, ptr(ws), ws.numel(), H._stream())


# (out_f, in_f, rows) -> the kernel the launcher documents: >= 512 rows per split = pipelined, fewer = two-barrier;
# out_f or in_f no multiple of 4 and no padded rows: no 16-byte loads, the f32 kernel (64 tile below 64 tiles of 128)
TN_SHAPES = [(1000, 516, 9001, 'tn_b3p'), (1000, 1100, 2001, 'tn_b3_128'), (1001, 516, 9001, 'tn_f32_64_slow'),
             (1000, 518, 9001, 'tn_f32_64_slow'), (1001, 1100, 2001, 'tn_f32_128_slow')]


@pytest.mark.parametrize('out_f,in_f,rows,variant', TN_SHAPES)
def test_tn_big_tile_tails(H, out_f, in_f, rows, variant):
    """The bf16-split kernels get the wide-range operands and the element-wise bar (their accumulator is updated once per
    16 rows: 48 roundings per 768-row split).  The f32 MFMA kernels update theirs once per 2 rows, ~1100 sequential
    roundings per split: with a dominant early row the partial sum stays at the error scale and the expected rounding
    error alone is eps/2 * sqrt(1100 / 3) ~ 6e-7 of it per element, ~2e-6 at the maximum over 5e5 elements (measured
    1.95e-6 at 1001 x 516 x 9001) -- the format's limit at that depth, no defect.  They are held to the bar the suite sets
    for these kernels, rel_err < 2e-6 on unit-variance operands (test_linear_fwd_bwd), where the same estimate gives 8e-7."""
    split = variant.startswith('tn_b3')
    g = gen(out_f + in_f + rows)
    dy = wide(g, rows, out_f, 2.0 if split else 0.0)
    x = wide(g, rows, in_f, 2.0 if split else 0.0)
    prior = torch.randn(out_f, in_f, generator=g)
    lddy, ldx = out_f + (8 if out_f % 4 == 0 else 7), in_f + (4 if in_f % 4 == 0 else 6)     # both multiples of 4
    dyd, xd = poison(dy, lddy), poison(x, ldx)
    ref = dy.double().t() @ x.double()
    scale = dy.double().abs().t() @ x.double().abs()
    for acc in (0, 1):
        dw = Out(out_f, in_f, prior if acc else None, flat=True)
        counted(H, variant, lambda: _wgrad(H, dyd, lddy, xd, ldx, dw, rows, in_f, out_f, acc=acc))
        got, r = dw.check(), ref + prior.double() if acc else ref
        if split:
            e = elem_err(got, r, scale + prior.double().abs() if acc else scale)
            assert e < 1e-6, (acc, e)
        else:
            assert rel_err(got, r) < 2e-6, acc


@pytest.mark.parametrize('M,N,R,variant', [(1001, 518, 9001, 'tn_b3p'), (1001, 1102, 2001, 'tn_b3_128')])
def test_tn_big_tile_padded_rows(H, M, N, R, variant):
    """ft_bgemm_tn with rows_padded: M and N no multiples of 4, the operands' rows readable (NaN here) up to the next
    multiple -- the 16-byte-load kernels; the NaN columns may only reach outputs that are masked.  The result is a column
    slice of a wider buffer (ldc)."""
    g = gen(M + N + R)
    a = torch.randn(R, M, generator=g)
    bm = torch.randn(R, N, generator=g)
    lda, ldb = (M + 3) // 4 * 4, (N + 3) // 4 * 4
    ad, bmd = poison(a, lda), poison(bm, ldb)
    ws = H.workspace(H._lib.query('ft_bgemm_tn_workspace', M, N, R, 1, 1), 'cuda')
    out = Out(M, N)
    counted(H, variant, lambda: _call('ft_bgemm_tn', ptr(ad), lda, 0, 0, ptr(bmd), ldb, 0, 0, out.ptr, out.ld, 0, 0, M, N, R,
                                      1, 1, 1, ptr(ws), ws.numel(), H._stream()))
    assert rel_err(out.check(), a.double().t() @ bm.double()) < 2e-6


@pytest.mark.parametrize('out_f,in_f,B,T,variant', [(1000, 516, 17, 529, 'tn_b3p'), (1000, 1100, 4, 501, 'tn_b3_128')])
@pytest.mark.parametrize('shift', [1, -1])
def test_tn_big_tile_time_major_shift(H, out_f, in_f, B, T, variant, shift):
    """recurrent-weight gradient form: both operands time-major, x read one step later / earlier (zero outside the item),
    T no multiple of 16"""
    rows = B * T
    g = gen(out_f + in_f + T + (shift > 0))
    dy = torch.randn(B, T, out_f, generator=g)
    x = torch.randn(B, T, in_f, generator=g)
    xs = torch.zeros_like(x)
    if shift > 0:
        xs[:, :T - shift] = x[:, shift:]
    else:
        xs[:, -shift:] = x[:, :T + shift]
    ref = dy.reshape(rows, out_f).double().t() @ xs.reshape(rows, in_f).double()
    lddy, ldx = out_f + 4, in_f + 8
    dyd = poison(_to_tm(dy.reshape(rows, out_f), B, T), lddy)
    xd = poison(_to_tm(x.reshape(rows, in_f), B, T), ldx)
    dw = Out(out_f, in_f, flat=True)
    counted(H, variant, lambda: _wgrad(H, dyd, lddy, xd, ldx, dw, rows, in_f, out_f, B, T, shift, 0, 1, 1))
    assert rel_err(dw.check(), ref) < 2e-6


# ---------------------------------------------------------------------------------------------------
# the other half of the split of responsibility: test_gpu_primitives.py's odd shapes are the 64-tile f32 kernels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,in_f,out_f,fwd,bwd,wgrad', [
    (130, 257, 66, 'rows_f32_64_nt_slow', 'rows_f32_64_nn_slow', 'tn_f32_64_slow'),
    (333, 10, 7, 'rows_f32_64_nt_slow', 'rows_f32_64_nn_slow', 'tn_f32_64_slow'),
    (4096, 256, 512, 'rows_f32_64_nt_fast', 'rows_f32_64_nt_fast', 'tn_f32_64_fast')])
def test_linear_fwd_bwd_shapes_land_on_the_64_tile(H, rows, in_f, out_f, fwd, bwd, wgrad):
    """assertion only: which kernels test_linear_fwd_bwd's shapes exercise (values are checked there)"""
    x = torch.randn(rows, in_f, device='cuda')
    w = torch.randn(out_f, in_f, device='cuda')
    dy = torch.randn(rows, out_f, device='cuda')
    counted(H, fwd, lambda: H.linear_fwd(x, w))
    counted(H, bwd, lambda: H.linear_bwd_data(dy, w))
    counted(H, wgrad, lambda: H.linear_bwd_weight(dy, x))
    torch.cuda.synchronize()
