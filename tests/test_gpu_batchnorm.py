"""BatchNorm statistics, apply, backward, the fused BatchNorm + MaxPool pair and the column sums (csrc/ft_bn.hip, and the
statistics epilogue of the 128x128 split GEMM in csrc/ft_gemm_b3.hip) against float64 (tests/bn_cpu.py, itself proven
against torch by tests/test_bn_cpu.py).

Every stage is compared with float64 GIVEN the fp32 values the stage before it actually produced -- statistics against
the y the GPU wrote, the apply kernels against the kernel's own save_mean / save_rstd, dy against the kernel's own
dgamma / dbeta -- so every tolerance is a rounding bound and an error of one stage cannot hide in another:

  sums (mean, dbeta, dgamma, column sums): accumulated in double, rounded to fp32 once:
        |got - ref| <= 2^-23 |ref| + 1e-12 sum|x|                      (fp32 accumulation does not meet this)
  statistics partials (doubles):  |got - ref| <= 1e-12 sum|x|
  rstd:  2^-23 rstd + the propagated 3e-12 E[y^2] error of the one-pass variance
  out:   8 * 2^-24 * (|xhat gamma| + |beta| + |residual|)              (at most 6 fp32 roundings)
  dy:    16 * 2^-24 * |gamma rstd| * (|g| + |dbeta| / n + |xhat dgamma| / n)
         (1 / n, the two products with it, xhat, two subtractions, gamma * rstd and the last product: <= 13 roundings,
          counting an fp32 division as 2.5 ulp)

dgamma's reference sums g * xhat with xhat = fp32((y - mean) * rstd), the product the kernel forms, in float64.
One comparison per test runs end to end from the original inputs, at the bound this layer already has in
test_bank_bn_pool_fused_equals_three_passes (rel_err < 2e-5).  Rows a kernel must not read (t >= tvalid(c)) hold NaN
and every result must be finite.  Each check prints its worst error over its bound (pytest -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cpu as R
from helpers import rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
E2E = 2e-5
EPS32 = float(np.float32(R.EPS))
B3_128 = ('rows_b3p', 'rows_b3_128')


@pytest.fixture(scope='module')
def H():
    from forwardtacotron_amd import hip
    assert torch.cuda.is_available()
    return hip


def query(name, *args):
    from forwardtacotron_amd import _lib
    return _lib.query(name, *args)


def dev(a, shift=False):
    """device copy of a numpy array; shift: its first element lies 4 bytes past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not shift:
        return t.cuda()
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device='cuda')
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def host(t):
    return t.detach().cpu().numpy()


def check(got, ref, bound, what):
    """every |got - ref| within its bound, got finite; prints and returns the worst error / bound"""
    got, ref = R.f64(got), R.f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = np.broadcast_to(R.f64(bound), ref.shape)
    assert np.all(np.isfinite(got)), f'{what}: non-finite result'
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(bound)), f'{what}: non-finite reference'
    ratio = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()) if got.size else 0.0
    print(f'    {what}: worst |err| / bound = {ratio:.3g}')
    assert ratio <= 1.0, f'{what}: error is {ratio:.3g} x its bound'
    return ratio


def e2e(got, ref, what):
    assert np.all(np.isfinite(R.f64(got))), what
    err = rel_err(torch.from_numpy(R.f64(got)), torch.from_numpy(R.f64(ref)))
    print(f'    {what}: end-to-end rel_err = {err:.3g} (bound {E2E:g})')
    assert err < E2E, (what, err)


def sum_bound(ref, sum_abs):
    return 2 * U * np.abs(ref) + 1e-12 * sum_abs


def variant_delta(H, fn):
    before = H.gemm_variant_counts()
    out = fn()
    after = H.gemm_variant_counts()
    return out, {k: after[k] - before[k] for k in after if after[k] != before[k]}


def plan_chunks(rows, C):
    """(chunks, rows per chunk) of the stand-alone column reduction: about 64 rows per chunk at least, at most
    clamp(1024 / column tiles, 16, 64) chunks, rows per chunk a multiple of 4"""
    want = min(max(1024 // max(-(-C // 64), 1), 16), 64)
    n = min(want, max(-(-rows // 64), 1))
    rpc = max(-(-(-(-rows // n)) // 4) * 4, 4)
    return max(-(-rows // rpc), 1), rpc


# ---------------------------------------------------------------------------------------------------
# stage checks
# ---------------------------------------------------------------------------------------------------
def check_statistics(y, mean, rstd, group, what):
    """save_mean / save_rstd against float64 statistics of the fp32 y the kernels read"""
    B, Tbuf, C = y.shape
    n = B * R.tvalid_all(C, Tbuf, group).astype(np.float64)
    m_ref, var, r_ref = R.stats(y, group, R.EPS)
    ab = R.abs_sums(y, group)                              # (sum |y|, sum y^2)
    mean_d = 1e-12 * ab[:, 0] / n                          # what the double sums may be off by
    var_d = 3e-12 * ab[:, 1] / n                           # E[y^2] - mean^2: both terms <= E[y^2]
    check(mean, m_ref, 2 * U * np.abs(m_ref) + mean_d, f'{what} mean')
    check(rstd, r_ref, 2 * U * r_ref + 0.5 * r_ref / (var + EPS32) * var_d, f'{what} rstd')
    return dict(n=n, mean=m_ref, var=var, rstd=r_ref, mean_d=mean_d, var_d=var_d)


def check_running(rm_new, rv_new, rm0, rv0, st, momentum, what):
    mo = float(np.float32(momentum))
    n = st['n']
    k = np.where(n > 1, n / np.maximum(n - 1, 1), 1.0)     # unbiased variance (n = 1: the biased one)
    ref_m = (1 - mo) * R.f64(rm0) + mo * st['mean']
    ref_v = (1 - mo) * R.f64(rv0) + mo * st['var'] * k
    check(rm_new, ref_m, 2 * U * np.abs(ref_m) + mo * st['mean_d'], f'{what} running_mean')
    check(rv_new, ref_v, 2 * U * np.abs(ref_v) + mo * k * st['var_d'], f'{what} running_var')


def check_apply(out, y, mean, rstd, gamma, beta, residual, what, pooled=False):
    """out against float64 from the kernel's own mean / rstd"""
    Tout = out.shape[1]
    ref = R.apply(y, mean, rstd, gamma, beta, residual, Tout)
    bound = 8 * U * (np.abs(R.xhat(R.f64(y)[:, :Tout], mean, rstd) * R.f64(gamma)) + np.abs(R.f64(beta)) +
                     (0.0 if residual is None else np.abs(R.f64(residual))))
    if pooled:                                            # max(a, b) moves by no more than a or b does
        ref, bound = R.pool(ref), R.pool(bound)
    check(out, ref, bound, f'{what} out')


def check_bwd(dy, dgamma, dbeta, g, y, gamma, mean, rstd, group, relu, what):
    """g [B, Tbuf, C]: the BatchNorm output's gradient, zero-padded beyond Tout -- exactly what the kernel sums;
    mean / rstd / dgamma / dbeta are the kernel's own fp32 values"""
    B, Tbuf, C = y.shape
    m = np.broadcast_to(R.valid_mask(Tbuf, C, group)[None], y.shape)
    ys = np.where(m, y, np.float32(0))
    g = np.where(m, R.f64(g), 0.0)
    xh32 = R.f64((ys - mean.astype(np.float32)) * rstd.astype(np.float32))          # fp32, as the kernel forms it
    assert ys.dtype == np.float32
    n = B * R.tvalid_all(C, Tbuf, group).astype(np.float64)
    ref_b = g.sum((0, 1))
    check(dbeta, ref_b, sum_bound(ref_b, np.abs(g).sum((0, 1))), f'{what} dbeta')
    p = np.where(m, g * xh32, 0.0)
    ref_g = p.sum((0, 1))
    check(dgamma, ref_g, sum_bound(ref_g, np.abs(p).sum((0, 1))), f'{what} dgamma')
    ref = R.bwd_apply(g, y, gamma, mean, rstd, dgamma, dbeta, group, relu)
    xh = np.where(m, R.xhat(ys, mean, rstd), 0.0)
    bound = 16 * U * np.abs(R.f64(gamma) * R.f64(rstd)) * (np.abs(g) + np.abs(R.f64(dbeta)) / n +
                                                            np.abs(xh * R.f64(dgamma)) / n)
    check(dy, ref, bound, f'{what} dy')
    assert np.all(dy[~m] == 0), f'{what}: dy beyond tvalid must be exactly 0'
    if relu:
        assert np.all(dy[m & ~(ys > 0)] == 0), f'{what}: dy where y <= 0 must be exactly 0'
    return ref


# ---------------------------------------------------------------------------------------------------
# a. statistics partials: GEMM epilogue, tap-split and stand-alone routes
# ---------------------------------------------------------------------------------------------------
def conv_ref(x, w, relu, Tout):
    """float64 Conv1d (padding k // 2, no bias) of channels-last x [B, T, Cin] with w [Cout, Cin, k] -> [B, Tout, Cout]"""
    y = F.conv1d(torch.from_numpy(R.f64(x)).transpose(1, 2), torch.from_numpy(R.f64(w)), padding=w.shape[2] // 2)
    y = y[:, :, :Tout].transpose(1, 2).numpy()
    return np.maximum(y, 0) if relu else y


def check_partials(part, nch, y, group, rpc, what):
    """every chunk's (sum, sum of squares) against float64 sums over exactly that chunk's valid rows of y"""
    B, Tbuf, C = y.shape
    P = host(part[:nch * C * 16].view(torch.float64).view(nch, C, 2))
    ref = R.chunk_partials(y, group, rpc, nch)
    mag = R.chunk_partials(np.abs(y), group, rpc, nch)
    check(P[..., 0], ref[..., 0], 1e-12 * mag[..., 0], f'{what} chunk sums ({nch} x {rpc} rows)')
    check(P[..., 1], ref[..., 1], 1e-12 * mag[..., 1], f'{what} chunk sums of squares')


def assert_route(route, delta, nch, B, Tbuf, C, what):
    print(f'    {what}: route {route}, {nch} chunks, GEMM variants {delta}')
    if route == 'epilogue':
        assert sum(delta.get(k, 0) for k in B3_128) == 1 and sum(delta.values()) == 1, delta
        assert nch == -(-B * Tbuf // 128)
        return 128
    if route == 'tapsplit':
        assert delta == {'rows_b3p': 1}, delta
    else:
        assert not any(k in delta for k in B3_128 + ('rows_b3p_ksplit',)), delta
    assert nch * C * 16 == query('ft_bn_workspace', B, Tbuf, C)
    n, rpc = plan_chunks(B * Tbuf, C)
    assert n == nch
    return rpc


def after_partials(H, part, nch, yd, yref64, group, Tout, rng, what):
    """bn_train_from_partials on the partials a conv left: statistics, apply, running stats, and end to end"""
    B, Tbuf, C = yd.shape
    gamma, beta = (rng.standard_normal(C).astype(np.float32) for _ in range(2))
    rm, rv = rng.standard_normal(C).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32)
    yp = torch.from_numpy(R.poison(host(yd), group)).cuda()          # same values, NaN where nothing may read
    rmd, rvd = dev(rm), dev(rv)
    out, mean, rstd = H.bn_train_from_partials(part, nch, yp, dev(gamma), dev(beta), rmd, rvd, Tout=Tout, group=group)
    y, mean, rstd = host(yp), host(mean), host(rstd)
    st = check_statistics(y, mean, rstd, group, what)
    check_running(host(rmd), host(rvd), rm, rv, st, H.BN_MOMENTUM, what)
    check_apply(host(out), y, mean, rstd, gamma, beta, None, what)
    if yref64 is not None:
        m64, _, r64 = R.stats(yref64, group, R.EPS)
        e2e(host(out), R.apply(yref64, m64, r64, gamma, beta, None, Tout), f'{what} out')


BANKS = [('epilogue', 96, 30, 16, 96, 8),      # Tbuf 31 < 64: the modulo form; 24 row tiles, the last with 32 rows; N edge at 96
         ('epilogue', 48, 63, 16, 128, 8),     # Tbuf 64: first size of the single-subtraction form
         ('epilogue', 47, 64, 16, 128, 8),     # Tbuf 65
         ('epilogue', 24, 128, 16, 128, 8),    # Tbuf 129 > a row tile
         ('alone', 3, 37, 12, 12, 5),
         ('alone', 2, 9, 8, 6, 4)]             # group 6: the scalar reduction


@pytest.mark.parametrize('route,B,T,Cin,C,K', BANKS)
def test_bank_statistics_partials(H, route, B, T, Cin, C, K):
    """conv_bank_fwd_stats: the members with 3, 5 and 7 taps end the pipelined kernel's stage loop on its three-stage
    tail; member i's statistics cover T rows for odd k and T + 1 for even k"""
    rng = np.random.default_rng(B * T)
    x = rng.standard_normal((B, T, Cin)).astype(np.float32)
    ws = [(0.2 * rng.standard_normal((C, Cin, k))).astype(np.float32) for k in range(1, K + 1)]
    wp_all = torch.cat([H.conv_pack_weight(dev(w)).reshape(-1) for w in ws])
    (yd, part, nch), delta = variant_delta(H, lambda: H.conv_bank_fwd_stats(dev(x), wp_all, K, C, relu=True))
    what = f'bank {(B, T, Cin, C, K)}'
    rpc = assert_route(route, delta, nch, B, T + 1, K * C, what)
    check_partials(part, nch, R.poison(host(yd), C), C, rpc, what)
    yref = np.full((B, T + 1, K * C), np.nan)
    for i, w in enumerate(ws):
        r = conv_ref(x, w, True, T + 1)
        yref[:, :r.shape[1], i * C:(i + 1) * C] = r
    assert np.array_equal(np.isnan(yref[0]), ~R.valid_mask(T + 1, K * C, C))
    after_partials(H, part, nch, yd, yref, C, T, rng, what)


CONVS = [('epilogue', 96, 128, 8, 256, 5, True),
         ('epilogue', 96, 128, 8, 192, 4, False),   # even k: Tout 129, 97 row tiles, half-filled second column tile
         ('tapsplit', 20, 128, 8, 256, 5, True),    # 40 tiles x 5 taps
         ('alone', 2, 9, 6, 8, 4, True)]


@pytest.mark.parametrize('route,B,T,Cin,Cout,k,relu', CONVS)
def test_conv_statistics_partials(H, route, B, T, Cin, Cout, k, relu):
    """conv1d_fwd_stats on its three routes; on the second shape again in bf16 mode, where the statistics must still
    describe the y that was written"""
    rng = np.random.default_rng(B * T + k)
    x = rng.standard_normal((B, T, Cin)).astype(np.float32)
    w = (0.2 * rng.standard_normal((Cout, Cin, k))).astype(np.float32)
    Tout = T + 1 - k % 2
    wp = H.conv_pack_weight(dev(w))
    what = f'conv {(B, T, Cin, Cout, k)}'
    if route == 'tapsplit':
        assert query('ft_conv1d_fwd_stats_workspace', B, Tout, Cout, k) > query('ft_conv_stats_workspace', B, Tout, Cout)
    (yd, part, nch), delta = variant_delta(H, lambda: H.conv1d_fwd_stats(dev(x), wp, relu, Tout))
    rpc = assert_route(route, delta, nch, B, Tout, Cout, what)
    check_partials(part, nch, host(yd), 0, rpc, what)
    after_partials(H, part, nch, yd, conv_ref(x, w, relu, Tout), 0, Tout - 1, rng, what)
    if (Cout, k) == (192, 4):
        y32 = yd.clone()
        with H.gemm_precision('bf16'):
            (yd, part, nch), delta = variant_delta(H, lambda: H.conv1d_fwd_stats(dev(x), wp, relu, Tout))
        rpc = assert_route(route, delta, nch, B, Tout, Cout, what + ' bf16')
        assert not torch.equal(yd, y32)
        assert rel_err(yd, y32) < 2e-2                       # bf16 operands: 2^-8 each
        check_partials(part, nch, host(yd), 0, rpc, what + ' bf16')
        after_partials(H, part, nch, yd, None, 0, Tout - 1, rng, what + ' bf16')


# ---------------------------------------------------------------------------------------------------
# b. bn_train_fwd, and the ordered finalize on host-built partials
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Tbuf,C,group', R.BN_CASES)
def test_bn_train_fwd(H, B, Tbuf, C, group):
    """16-byte and scalar kernels (C, group, a y that starts 4 bytes past a 16-byte boundary), Tout < Tbuf, residual,
    two momenta, running stats from random values; channel 0 is constant, channel 1 has mean 100 / std 1"""
    a, gamma, beta, rm, rv = R.bn_inputs(B, Tbuf, C, group, seed=B * 1000 + Tbuf)
    nchunks = query('ft_bn_workspace', B, Tbuf, C) // (C * 16)
    assert nchunks == plan_chunks(B * Tbuf, C)[0] == R.BN_CHUNKS.get((B, Tbuf, C, group), nchunks)
    rng = np.random.default_rng(7)
    for shift, with_res, momentum in ((False, True, 0.1), (True, False, 0.37), (True, True, 0.1)):
        Tout = Tbuf - 1 if group > 0 else (Tbuf if with_res else max(Tbuf - 2, 1))
        res = rng.standard_normal((B, Tout, C)).astype(np.float32) if with_res else None
        rmd, rvd = dev(rm), dev(rv)
        out, mean, rstd = H.bn_train_fwd(dev(a, shift), dev(gamma), dev(beta), rmd, rvd, Tout, group,
                                         residual=None if res is None else dev(res, shift),
                                         momentum=momentum)
        what = f'bn_train_fwd {(B, Tbuf, C, group)} {nchunks} chunks shift={shift} Tout={Tout} m={momentum}'
        mean, rstd = host(mean), host(rstd)
        st = check_statistics(a, mean, rstd, group, what)
        check_running(host(rmd), host(rvd), rm, rv, st, momentum, what)
        check_apply(host(out), a, mean, rstd, gamma, beta, res, what)
        e2e(host(out), R.apply(a, st['mean'], st['rstd'], gamma, beta, res, Tout), f'{what} out')
        assert mean[0] == np.float32(0.75) and st['var'][0] == 0           # the constant channel, through the clamp
        assert abs(rstd[0] * np.sqrt(EPS32) - 1) <= 2 * U
        if B * Tbuf == 1:                                   # n = 1: variance 0, unbiased = biased
            assert np.array_equal(mean, a[0, 0]) and np.all(st['var'] == 0)


@pytest.mark.parametrize('nchunks', [1, 7, 8, 9, 65])
def test_finalize_from_host_partials(H, nchunks):
    """bn_train_from_partials / bn_pool_from_partials on float64 partials built on the host: the exact sums of y split
    over nchunks uneven row ranges (8 lanes finalize a column), plus one channel whose E[y^2] - mean^2 is negative"""
    B, Tbuf, C, group = 5, 27, 40, 4
    rows = np.array_split(np.arange(B * Tbuf), nchunks)

    def split(y):
        v = np.where(R.valid_mask(Tbuf, C, group)[None], R.f64(y), 0.0).reshape(B * Tbuf, C)
        return np.stack([np.stack([v[r].sum(0), (v[r] ** 2).sum(0)], axis=1) for r in rows])

    a, gamma, beta, rm, rv = R.bn_inputs(B, Tbuf, C, group, seed=nchunks)
    part = split(a)
    part[:, 0, 1] *= 1 - 1e-9                               # channel 0 is constant: its variance is now -5.6e-10
    rmd, rvd = dev(rm), dev(rv)
    out, mean, rstd = H.bn_train_from_partials(dev(part), nchunks, dev(a), dev(gamma), dev(beta), rmd, rvd,
                                               Tout=Tbuf - 1, group=group, momentum=0.37)
    what = f'host partials x{nchunks}'
    m_ref, r_ref, rm_ref, rv_ref = R.finalize(part, B, Tbuf, group, 0.37, R.EPS, rm, rv)
    assert r_ref[0] == 1 / np.sqrt(EPS32)
    check(mean, m_ref, 2 * U * np.abs(m_ref), f'{what} mean')
    check(rstd, r_ref, 2 * U * r_ref, f'{what} rstd')
    check(rmd, rm_ref, 2 * U * np.abs(rm_ref), f'{what} running_mean')
    check(rvd, rv_ref, 2 * U * np.abs(rv_ref), f'{what} running_var')
    check_apply(host(out), a, host(mean), host(rstd), gamma, beta, None, what)

    y, gamma, beta, _ = R.pool_inputs(B, Tbuf, Tbuf - 1, C, group, seed=nchunks)
    part = split(y)
    rmd, rvd = dev(rm), dev(rv)
    out, mean, rstd = H.bn_pool_from_partials(dev(part), nchunks, dev(y), dev(gamma), dev(beta), rmd, rvd,
                                              Tout=Tbuf - 1, group=group)
    what = f'host partials x{nchunks}, pooled'
    m_ref, r_ref, rm_ref, rv_ref = R.finalize(part, B, Tbuf, group, H.BN_MOMENTUM, R.EPS, rm, rv)
    check(mean, m_ref, 2 * U * np.abs(m_ref), f'{what} mean')
    check(rstd, r_ref, 2 * U * r_ref, f'{what} rstd')
    check(rmd, rm_ref, 2 * U * np.abs(rm_ref), f'{what} running_mean')
    check(rvd, rv_ref, 2 * U * np.abs(rv_ref), f'{what} running_var')
    check_apply(host(out), y, host(mean), host(rstd), gamma, beta, None, what, pooled=True)


# ---------------------------------------------------------------------------------------------------
# c. bn_bwd
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Tbuf,C,group', R.BN_CASES)
@pytest.mark.parametrize('relu', [False, True])
def test_bn_bwd(H, B, Tbuf, C, group, relu):
    """dgamma / dbeta / dy on both kernel forms; y = relu(a) from fp32 a, so the mask is exact.  A bank's even-k member
    has Tout = Tbuf - 1: its last row gets no dout but counts in the statistics, so its dy is not zero"""
    a, gamma, _, _, _ = R.bn_inputs(B, Tbuf, C, group, seed=B * 1000 + Tbuf)
    y = np.maximum(a, np.float32(0)) if relu else a
    Tout = Tbuf - 1 if group > 0 else Tbuf
    dout = np.random.default_rng(11).standard_normal((B, Tout, C)).astype(np.float32)
    g = np.zeros((B, Tbuf, C))
    g[:, :Tout] = dout
    m64, _, r64 = R.stats(y, group, R.EPS)
    for shift in (False, True):
        _, mean, rstd = H.bn_train_fwd(dev(y), dev(gamma), dev(gamma), None, None, Tout, group)
        dy, dgamma, dbeta = H.bn_bwd(dev(dout, shift), dev(y, shift), dev(gamma), mean, rstd, group, relu)
        what = f'bn_bwd {(B, Tbuf, C, group)} relu={relu} shift={shift}'
        dy, dgamma, dbeta = host(dy), host(dgamma), host(dbeta)
        ref = check_bwd(dy, dgamma, dbeta, g, y, gamma, host(mean), host(rstd), group, relu, what)
        if group > 0 and B * Tbuf > 8:                      # the sliced-off row of the even-k members
            even = R.tvalid_all(C, Tbuf, group) == Tbuf
            assert even.any() and np.count_nonzero(ref[:, Tout:, even]) > 0
            assert np.array_equal(dy[:, Tout:, even] != 0, ref[:, Tout:, even] != 0)
        want = R.bwd(dout, y, gamma, m64, r64, group, relu)
        for got, w, name in zip((dy, dgamma, dbeta), want, ('dy', 'dgamma', 'dbeta')):
            e2e(got, w, f'{what} {name}')


# ---------------------------------------------------------------------------------------------------
# d. BatchNorm + MaxPool1d(2, 1, 1) fused
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Tbuf,Tout,C,group', R.POOL_CASES)
@pytest.mark.parametrize('relu', [False, True])
def test_bn_pool_fwd_bwd(H, B, Tbuf, Tout, C, group, relu):
    """bn_pool_from_partials / bn_pool_bwd, every element compared: the inputs (bn_cpu.pool_inputs) keep every pooling
    decision more than 1e-3 away from flipping and make the ties exact, which tests/test_bn_cpu.py asserts"""
    y, gamma, beta, dout = R.pool_inputs(B, Tbuf, Tout, C, group, seed=Tbuf)
    part = R.chunk_partials(y, group, -(-B * Tbuf // 3), 3)
    out, mean, rstd = H.bn_pool_from_partials(dev(part), 3, dev(y), dev(gamma), dev(beta), None, None, Tout=Tout,
                                              group=group)
    what = f'bn_pool {(B, Tbuf, Tout, C, group)} relu={relu}'
    st = check_statistics(y, host(mean), host(rstd), group, what)
    check_apply(host(out), y, host(mean), host(rstd), gamma, beta, None, what, pooled=True)
    e2e(host(out), R.pool(R.apply(y, st['mean'], st['rstd'], gamma, beta, None, Tout)), f'{what} out')
    assert R.pool_min_gap(R.apply(y, host(mean), host(rstd), gamma, beta, None, Tout))[0] > 1e-3

    dy, dgamma, dbeta = H.bn_pool_bwd(dev(dout), dev(y), dev(gamma), dev(beta), mean, rstd, group, relu)
    dy, dgamma, dbeta = host(dy), host(dgamma), host(dbeta)
    dz = R.pool_dz(dout, y, gamma, beta, host(mean), host(rstd))
    assert np.array_equal(dz, dz.astype(np.float32))        # sums of two multiples of 1/16: exact in fp32
    g = np.zeros((B, Tbuf, C))
    g[:, :Tout] = dz
    check_bwd(dy, dgamma, dbeta, g, y, gamma, host(mean), host(rstd), group, relu, what)
    want = R.pool_bwd(dout, y, gamma, beta, st['mean'], st['rstd'], group, relu)
    for got, w, name in zip((dy, dgamma, dbeta), want, ('dy', 'dgamma', 'dbeta')):
        e2e(got, w, f'{what} {name}')


# ---------------------------------------------------------------------------------------------------
# e. column sums and the eval-mode fold
# ---------------------------------------------------------------------------------------------------
def wide_matrix(rng, rows, C, ld, e0):
    """flat device buffer holding M [rows, ld] from element `e0 - col0` on; returns (buffer, float64 view of the C
    columns that start at flat element e0).  The last of those columns is 1000 + noise."""
    flat = rng.standard_normal(rows * ld + e0 + 8).astype(np.float32)
    cols = flat[e0:e0 + rows * ld].reshape(rows, ld)[:, :C] if rows * ld else np.zeros((rows, C), np.float32)
    if C and rows:
        cols[:, C - 1] += np.float32(1000)
    return dev(flat), R.f64(cols)


def check_colsum(got, ref64, scale, old, what):
    ref = scale * ref64.sum(0) + (0.0 if old is None else R.f64(old))
    extra = 0.0 if old is None else 2 * U * np.abs(scale * ref64.sum(0))       # fp32(scale * sum), then one fp32 addition
    check(got, ref, sum_bound(ref, abs(scale) * np.abs(ref64).sum(0)) + extra, what)


@pytest.mark.parametrize('rows', [0, 1, 63, 65, 4097, 26912])
def test_colsum(H, rows):
    """ft_colsum: 16-byte and scalar kernels, a column slice of a wider matrix (ldx > C), an unaligned base, scale and
    accumulate; 26,912 rows of 1000 + noise is where fp32 accumulation would miss the bound"""
    rng = np.random.default_rng(rows)
    for C in (0, 4, 6, 260) if rows != 26912 else (8, 6):
        for ld, e0, scale, acc in ((C, 0, 1.0, False), (C + 8, 4, -0.5, True), (C + 8, 3, 1.0, False),
                                   (C + 3, 0, 2.0, True)):
            buf, cols = wide_matrix(rng, rows, C, ld, e0)
            old = rng.standard_normal(C).astype(np.float32) if acc else None
            out = dev(old) if acc else torch.full((C,), float('nan'), device='cuda')
            H.colsum_raw(buf.data_ptr() + 4 * e0, ld, out, rows, C, scale, acc)
            check_colsum(out, cols, scale, old, f'colsum rows={rows} C={C} ld={ld} base+{e0} scale={scale} acc={acc}')
    x = rng.standard_normal((3, max(rows, 1), 12)).astype(np.float32)
    check_colsum(H.colsum(dev(x)), R.f64(x).reshape(-1, 12), 1.0, None, f'colsum [3, {max(rows, 1)}, 12]')


@pytest.mark.parametrize('rows,C,ld,e0', [(4097, 260, 268, 4), (65, 4, 4, 0), (26912, 8, 8, 0), (4097, 6, 14, 3),
                                          (63, 260, 268, 1), (1, 4, 7, 0), (0, 4, 4, 0)])
def test_colsum2(H, rows, C, ld, e0):
    """two matrices in one launch (16-byte lanes) and the two-call fallback (C % 4, ldx % 4, base alignment, no rows)"""
    rng = np.random.default_rng(rows + C)
    b0, c0 = wide_matrix(rng, rows, C, ld, e0)
    b1, c1 = wide_matrix(rng, rows, C, ld, e0)
    o0, o1 = (torch.full((C,), float('nan'), device='cuda') for _ in range(2))
    H.colsum2_raw(b0.data_ptr() + 4 * e0, b1.data_ptr() + 4 * e0, ld, o0, o1, rows, C)
    check_colsum(o0, c0, 1.0, None, f'colsum2[0] rows={rows} C={C} ld={ld} base+{e0}')
    check_colsum(o1, c1, 1.0, None, f'colsum2[1] rows={rows} C={C} ld={ld} base+{e0}')


@pytest.mark.parametrize('rows,Cs', [(4097, (4, 260, 64, 8)), (4097, (4, 6, 260)), (1, (4, 8)), (26912, (8, 4))])
def test_colsum_batch(H, rows, Cs):
    """several matrices in one launch, and the one-call-each fallback (a C that is no multiple of 4); every result is
    also bit-equal to its own colsum"""
    rng = np.random.default_rng(rows + len(Cs))
    xs = [rng.standard_normal((rows, C)).astype(np.float32) for C in Cs]
    for x in xs:
        x[:, -1] += np.float32(1000)
    xd = [dev(x) for x in xs]
    outs = H.colsum_batch(xd)
    for x, d, o in zip(xs, xd, outs):
        check_colsum(o, R.f64(x), 1.0, None, f'colsum_batch rows={rows} C={x.shape[1]} of {Cs}')
        assert torch.equal(o, H.colsum(d))


@pytest.mark.parametrize('C', [1, 70, 260])
def test_bn_fold_eval(H, C):
    """scale = gamma / sqrt(rv + eps): an fp32 addition, a square root and a division (2.5 ulp if not correctly rounded)
    -> 8 * 2^-24; shift = beta - rm * scale adds a product and a subtraction"""
    _, gamma, beta, rm, rv = R.bn_inputs(1, 2, C, 0, seed=C)
    scale, shift = H.bn_fold_eval(dev(gamma), dev(beta), dev(rm), dev(rv))
    s_ref, h_ref = R.fold_eval(gamma, beta, rm, rv, R.EPS)
    check(scale, s_ref, 8 * U * np.abs(s_ref), f'fold C={C} scale')
    check(shift, h_ref, 10 * U * (np.abs(R.f64(beta)) + np.abs(R.f64(rm) * s_ref)), f'fold C={C} shift')
