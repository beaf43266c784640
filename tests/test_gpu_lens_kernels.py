"""GPU: the small length-aware kernels under every generate_batch, each alone through its hip.py wrapper against
tests/lens_cpu.py (plain numpy; proven against torch by tests/test_lens_cpu.py, which also holds the properties of the
edge tables used here):

  conv1d_bias_fwd_lens    the BIAS arm of the GEMM epilogues under the row mask: ft_gemm_rows_kernel (ft_gemm.hip) and
                          rows_b3_epilogue<1, 1> / <2, 2> (ft_gemm_b3.hip), each path proven by hip.gemm_variant_counts()
  add_layernorm_fwd_lens  ft_add_layernorm_fwd_lens_kernel
  transpose_pad_lens_fwd  ft_transpose_pad_lens_kernel
  gen_durations, lr_scan  ft_gen_durations_kernel with ft_lr_scan_kernel: mel_len must be the scan's total
  check_tokens_lens       ft_check_tokens_lens_kernel

Every comparison is exact equality or a rounding bound derived from the formats (lens_cpu.conv_f32_bound, conv_b3_bound,
layernorm_bound: the derivations stand there); each bounded check prints its worst error / bound (pytest -s).  Rows a
kernel must not read hold NaN.  No NaN or out-of-range value sits inside j < x_len[b] of a duration row: the conversion
of those to an integer is unspecified and nothing here pins it.

Not covered: rows_b3_128 and rows_f32_128_* under the mask.  They are reachable only with FT_GEMM_PIPE=0 / FT_GEMM_B3=0,
which the library reads once per process."""
import numpy as np
import pytest
import torch

import lens_cpu as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def H():
    from forwardtacotron_amd import hip
    assert torch.cuda.is_available()
    return hip


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def worst(got, want, bound, keep, what):
    ratio = float((np.abs(R.f64(got) - want) / bound)[keep].max())
    print(f'    {what}: worst |err| / bound = {ratio:.3f}')
    assert np.all(np.isfinite(got)), what
    assert ratio <= 1.0, f'{what}: error is {ratio:.3g} x its bound'


# ---- conv1d_bias_fwd_lens --------------------------------------------------------------------------------------------
def conv_case(H, T, lens, Cin, Cout, k, relu, precision, variant, seed):
    from forwardtacotron_amd.fastpitch import ConvBiasFn
    B = len(lens)
    g = np.random.default_rng(seed)
    valid = R.valid_rows(lens, T)
    x = (g.standard_normal((B, T, Cin)) * valid[:, :, None]).astype(np.float32)       # the contract: zero past the length
    w = (g.standard_normal((Cout, Cin, k)) * 0.3).astype(np.float32)
    bias = (np.where(g.random(Cout) < 0.5, -1.0, 1.0) * (0.5 + g.random(Cout))).astype(np.float32)
    assert (bias > 0).any() and (bias < 0).any()
    xn = x.copy()                         # NaN wherever no valid row reaches: t >= lens[b] + k // 2
    xn[np.arange(T)[None, :] >= np.asarray(lens)[:, None] + k // 2] = np.nan
    above = torch.tensor([T + 5 if L == T else L for L in lens])
    assert np.isnan(xn).any() and int(above.max()) > T
    xd, wd, bd, ld = dev(x), dev(w), dev(bias), torch.tensor(lens).cuda()
    wp = H.conv_pack_weight(wd)
    with H.gemm_precision(precision), torch.no_grad():
        c0 = H.gemm_variant_counts()
        y = H.conv1d_bias_fwd_lens(xd, wp, bd, relu, ld)
        c1 = H.gemm_variant_counts()
        plain = ConvBiasFn.apply(xd, wd, bd, relu)
        c2 = H.gemm_variant_counts()
        y_nan = H.conv1d_bias_fwd_lens(dev(xn), wp, bd, relu, ld)
        y_above = H.conv1d_bias_fwd_lens(xd, wp, bd, relu, above.cuda())
    took = {v: c1[v] - c0[v] for v in c1 if c1[v] != c0[v]}
    assert took == {variant: 1}, took
    assert took == {v: c2[v] - c1[v] for v in c2 if c2[v] != c1[v]}, 'the unmasked launch took another kernel'
    y, plain, y_nan, y_above = host(y), host(plain), host(y_nan), host(y_above)
    bf16 = precision == 'bf16'
    want, mag = R.conv_bias_lens(x, w, bias, relu, lens, bf16=bf16)
    bound = R.conv_f32_bound(mag, Cin, k) if variant.startswith('rows_f32') else R.conv_b3_bound(mag, bias, Cin, k, bf16)
    worst(y, want, bound, valid, f'{variant} {precision} Cin {Cin} k {k} relu {relu}')
    assert np.all(bits(y[~valid]) == 0), 'masked rows must be +0.0: not bias, relu(bias) or -0.0'
    assert np.array_equal(bits(y[valid]), bits(plain[valid])), 'valid rows must be bit-equal to the unmasked launch'
    assert (plain[~valid] != 0).any(), 'the unmasked launch leaves the padding non-zero: the mask has work'
    assert np.array_equal(bits(y_nan), bits(y)), 'rows of x at t >= lens[b] + k // 2 reached the output'
    assert np.array_equal(bits(y_above), bits(y)), 'a length above T must behave as T'


@pytest.mark.parametrize('k,relu', [(1, False), (3, True), (9, False)])
def test_conv_bias_lens_small_fp32(H, k, relu):
    """ft_gemm_rows_kernel's epilogue (64-row tiles, 16-byte operand loads); ReLU off is the FFTBlock's second
    convolution, whose masked rows would otherwise hold the bias"""
    conv_case(H, R.T_SMALL, R.LENS_SMALL, 8, 10, k, relu, 'fp32', 'rows_f32_64_nt_fast', 100 + k)


def test_conv_bias_lens_small_fp32_slow(H):
    """K = Cin = 7 is no multiple of 4: the scalar-load form of the same kernel"""
    conv_case(H, R.T_SMALL, R.LENS_SMALL, 7, 10, 3, False, 'fp32', 'rows_f32_64_nt_slow', 110)


@pytest.mark.parametrize('k', [1, 9])
def test_conv_bias_lens_small_bf16(H, k):
    """rows_b3_epilogue<1, 1>: 16 keep bits per lane"""
    conv_case(H, R.T_SMALL, R.LENS_SMALL, 8, 10, k, False, 'bf16', 'rows_b3_64', 120 + k)


@pytest.mark.parametrize('Cin,k,relu,precision', [(8, 9, False, 'fp32'), (8, 3, True, 'fp32'), (40, 3, False, 'fp32'),
                                                  (8, 1, False, 'bf16')])
def test_conv_bias_lens_large(H, Cin, k, relu, precision):
    """rows_b3_epilogue<2, 2> of the pipelined 128-row kernel: 32 keep bits per lane; Cin = 40 leaves a K tail of 8 in the
    16-deep MFMA stage of every tap"""
    conv_case(H, R.T_BIG, R.LENS_BIG, Cin, R.COUT_BIG, k, relu, precision, 'rows_b3p', 130 + Cin + k)


# ---- add_layernorm_fwd_lens ------------------------------------------------------------------------------------------
def layernorm_case(H, D, has_res, offset, lens):
    from forwardtacotron_amd import _lib
    from forwardtacotron_amd.fastpitch import AddLayerNormFn
    B, T = R.LN_B, R.LN_T
    x, res, gamma, beta = R.layernorm_inputs(D, has_res, offset)
    valid = R.valid_rows(lens, T)
    xn, rn = x.copy(), None if res is None else res.copy()
    xn[~valid] = np.nan
    if has_res:
        rn[~valid] = np.nan
    gd, bd, ld = dev(gamma), dev(beta), torch.tensor(lens).cuda()
    with torch.no_grad():
        y = host(H.add_layernorm_fwd_lens(dev(x), dev(res) if has_res else None, gd, bd, ld, R.LN_EPS))
        y_nan = host(H.add_layernorm_fwd_lens(dev(xn), dev(rn) if has_res else None, gd, bd, ld, R.LN_EPS))
        train = host(AddLayerNormFn.apply(dev(x), dev(res) if has_res else None, gd, bd, R.LN_EPS))
        # the same entry point onto an output buffer that holds NaN: the masked rows are stored, not left
        xd, rd = dev(xn), dev(rn) if has_res else None
        into = torch.full((B, T, D), float('nan'), device='cuda')
        _lib.call('ft_add_layernorm_fwd_lens', xd.data_ptr(), rd.data_ptr() if has_res else None, gd.data_ptr(),
                  bd.data_ptr(), ld.data_ptr(), into.data_ptr(), B, T, D, float(R.LN_EPS), H._stream())
        into = host(into)
    want, smax, sigma, xhat = R.add_layernorm_lens(x, res, gamma, beta, lens, R.LN_EPS)
    bound = R.layernorm_bound(want, smax, sigma, xhat, gamma, R.LN_EPS, D, has_res)
    if valid.any():
        worst(y, want, bound, valid, f'D {D} res {has_res} offset {offset} lens {lens}')
    assert np.array_equal(bits(y[valid]), bits(train[valid])), 'valid rows must be bit-equal to the training kernel (p = 0)'
    assert np.all(bits(y[~valid]) == 0), 'masked rows must be +0.0, not beta'
    assert (train[~valid] != 0).all(), 'LayerNorm turns a zero row into beta: the mask has work'
    assert np.array_equal(bits(y_nan), bits(y)), 'x / res past the length reached the output'
    assert np.array_equal(bits(into), bits(y)), 'a row was left as the output buffer held it'


@pytest.mark.parametrize('offset', [False, True])
@pytest.mark.parametrize('has_res', [True, False])
@pytest.mark.parametrize('D', R.LN_DIMS)
def test_add_layernorm_lens(H, D, has_res, offset):
    layernorm_case(H, D, has_res, offset, R.LN_LENS)


def test_add_layernorm_lens_empty_item_and_length_above_T(H):
    layernorm_case(H, 130, True, False, R.LN_LENS_EDGE)


# ---- transpose_pad_lens_fwd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', [R.PAD, 0.0])
@pytest.mark.parametrize('B,T,C,Tout', R.TP_SHAPES)
def test_transpose_pad_lens(H, B, T, C, Tout, pad):
    x = np.random.default_rng(T * 100 + C).standard_normal((B, T, C)).astype(np.float32)
    x[x == 0] = 1.0
    full = host(H.transpose_pad_fwd(dev(x), Tout, pad))
    for lens in R.transpose_lens_sets(B, T):
        xn = x.copy()
        xn[~R.valid_rows(lens, T)] = np.nan
        want = R.transpose_pad_lens(x, lens, Tout, pad)
        assert np.array_equal(bits(want), bits(R.transpose_pad_lens(xn, lens, Tout, pad))) and np.all(np.isfinite(want))
        got = host(H.transpose_pad_lens_fwd(dev(xn), torch.tensor(lens).cuda(), Tout, pad))
        assert np.all(np.isfinite(got)), f'lens {lens}: x past the length came through'
        assert np.array_equal(bits(got), bits(want)), f'lens {lens}'
        for b, L in enumerate(lens):
            if L == T:
                assert np.array_equal(bits(got[b]), bits(full[b])), 'a full item must be transpose_pad_fwd\'s'


# ---- gen_durations with lr_scan --------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_range', [False, True])
@pytest.mark.parametrize('Tx', R.DUR_TX)
def test_gen_durations_and_scan(H, Tx, in_range):
    names, dur, x_len = R.duration_table(Tx, in_range)
    want, want_len, want_bad = R.gen_durations(dur, x_len)
    assert want_bad == (0 if in_range else 1)
    d = dev(dur)
    mel_len, bad = H.gen_durations(d, dev(x_len))
    got = host(d)                                                         # in place
    for b, name in enumerate(names):
        assert np.array_equal(got[b], want[b]), (name, got[b], want[b])
    assert np.array_equal(host(mel_len), want_len), (names, host(mel_len), want_len)
    assert int(bad.item()) == want_bad
    cum, total = H.lr_scan(d)
    wcum, wtotal = R.lr_scan(got)
    assert np.array_equal(host(total).astype(np.int64), host(mel_len)), 'mel_len must be the scan\'s total'
    for b, name in enumerate(names):
        assert np.array_equal(host(cum)[b], wcum[b]), name
    assert np.array_equal(host(total), wtotal) and np.array_equal(host(d), got), 'the scan found something to clamp'


# ---- check_tokens_lens -----------------------------------------------------------------------------------------------
def test_check_tokens_lens(H):
    B, T, lens = R.TOK_B, R.TOK_T, R.TOK_LENS
    ld = torch.tensor(lens).cuda()
    idx = np.random.default_rng(9).integers(1, 50, (B, T)).astype(np.int64)
    idx[~R.valid_rows(lens, T)] = 0                                       # zeros only in the padding

    def run(ids, start):
        flag = torch.full((1,), start, dtype=torch.int32, device='cuda')
        H.check_tokens_lens(dev(ids), ld, flag)
        assert int(flag.item()) == start | R.check_tokens(ids, lens)
        return int(flag.item())

    assert run(idx, 0) == 0
    inside = idx.copy()
    inside[B - 1, lens[-1] - 1] = 0                                       # the last valid token of the last item
    assert run(inside, 0) == 2
    assert run(inside, 1) == 3, 'the kernel ORs into the flag word'
    behind = idx.copy()
    behind[B - 1, lens[-1] - 1], behind[B - 1, lens[-1]] = 7, 0           # the same zero one token on: in the padding
    assert run(behind, 0) == 0 and run(behind, 1) == 1
