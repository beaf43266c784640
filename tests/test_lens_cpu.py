"""CPU: tests/lens_cpu.py itself.  The float restatements equal torch's float64 conv1d / layer_norm run item by item on
x[b, :L] to 1e-12; the duration functions equal a per-item torch float32 evaluation of the reference's own statements
(`d.long().sum() <= 0`, `fill 2.`, `d[d < 0] = 0`, `(d + 0.5).long()`) bit for bit; the LayerNorm error bound holds for
torch's own fp32 layer_norm on the GPU test's inputs (it is not too tight for a reasonable fp32 implementation); and every
row of the GPU tests' edge tables has the property that makes it an edge."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lens_cpu as R

f32 = np.float32


# ---- convolution with bias -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cin,k,relu', [(8, 1, False), (8, 3, True), (8, 9, False), (7, 3, False), (5, 5, True)])
def test_conv_bias_lens_equals_torch_per_item(Cin, k, relu):
    T, lens, Cout = R.T_SMALL, R.LENS_SMALL, 10
    g = torch.Generator().manual_seed(k * 10 + Cin)
    x = torch.randn(len(lens), T, Cin, generator=g, dtype=torch.float64)
    x = x * (torch.arange(T)[None, :, None] < torch.tensor(lens)[:, None, None])
    w = torch.randn(Cout, Cin, k, generator=g, dtype=torch.float64)
    bias = torch.randn(Cout, generator=g, dtype=torch.float64)
    want, mag = R.conv_bias_lens(x, w, bias, relu, lens)
    wabs, magabs = R.conv_bias_lens(x.abs(), w.abs(), bias.abs(), False, lens)
    for b, L in enumerate(lens):
        y = F.conv1d(x[b:b + 1, :L].transpose(1, 2), w, bias, padding=k // 2).transpose(1, 2)[0]
        y = torch.relu(y) if relu else y
        assert np.abs(want[b, :L] - y.numpy()).max() <= 1e-12
        assert not want[b, L:].any() and not mag[b, L:].any()
    assert np.abs(mag - wabs).max() <= 1e-12 and np.abs(magabs - wabs).max() <= 1e-12    # mag = the sum over |.|
    assert np.all(np.abs(want) <= mag + 1e-12)
    above = R.conv_bias_lens(x, w, bias, relu, [T + 5 if L == T else L for L in lens])[0]
    assert np.array_equal(above, want), 'a length above T is T'


def test_bf16_rounding_is_torchs():
    g = torch.Generator().manual_seed(3)
    a = torch.cat([torch.randn(4096, generator=g) * 3, torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0, 2.0 ** -130])])
    assert np.array_equal(R.bf16_round(a.numpy()).view(np.uint32), a.bfloat16().float().numpy().view(np.uint32))
    x = torch.randn(2, 5, 3, generator=g)
    w = torch.randn(4, 3, 3, generator=g)
    bias = torch.randn(4, generator=g)
    got = R.conv_bias_lens(x, w, bias, False, [5, 3], bf16=True)[0]
    ref = R.conv_bias_lens(x.bfloat16().float(), w.bfloat16().float(), bias, False, [5, 3])[0]
    assert np.array_equal(got, ref) and not np.array_equal(got, R.conv_bias_lens(x, w, bias, False, [5, 3])[0])


def test_conv_tile_geometry():
    """the item ends against the 64- and 128-row tiles, as test_gpu_generate_batch_paths.py asserts them"""
    T, L = R.T_SMALL, R.LENS_SMALL
    assert T + L[1] - 1 == 64 and 3 * T + L[3] == 128 and L[0] == T and L[2] == 1
    T, L = R.T_BIG, R.LENS_BIG
    assert len(L) * T >= 96 * 128 and R.COUT_BIG == 2 * 128           # 192 tiles: the launcher takes the 128-row kernel
    assert (L[0] - 1) % 128 == 0 and (T + L[1]) % 128 == 0 and L[2] == 1 and L[3] == T
    assert (4 * T + L[4]) % 128 == 121 and (len(L) * T) % 128 == 112


# ---- add + LayerNorm -----------------------------------------------------------------------------------------------
LN_CASES = [(D, has_res, offset) for D in R.LN_DIMS for has_res in (True, False) for offset in (False, True)]


@pytest.mark.parametrize('D,has_res,offset', LN_CASES)
@pytest.mark.parametrize('lens', [R.LN_LENS, R.LN_LENS_EDGE])
def test_add_layernorm_lens_equals_torch_per_item(D, has_res, offset, lens):
    x, res, gamma, beta = R.layernorm_inputs(D, has_res, offset)
    xn = x.copy()
    xn[~R.valid_rows(lens, R.LN_T)] = np.nan                             # never read past the length
    want, smax, sigma, xhat = R.add_layernorm_lens(xn, res, gamma, beta, lens, R.LN_EPS)
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(sigma))
    eps = float(f32(R.LN_EPS))
    for b, L in enumerate(lens):
        L = min(L, R.LN_T)
        s = torch.from_numpy(x[b, :L]).double() + (torch.from_numpy(res[b, :L]).double() if has_res else 0.0)
        y = F.layer_norm(s, (D,), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), eps)
        assert L == 0 or np.abs(want[b, :L] - y.numpy()).max() <= 1e-12
        assert not want[b, L:].any()


@pytest.mark.parametrize('D,has_res,offset', LN_CASES)
def test_layernorm_bound_holds_for_torch_fp32(D, has_res, offset):
    """sanity of the bound: torch's CPU fp32 layer_norm of fp32 (x + res) stays inside it -- and the bound is tight
    enough to see a one-pass variance at the + 100 rows"""
    x, res, gamma, beta = R.layernorm_inputs(D, has_res, offset)
    lens = [R.LN_T] * R.LN_B
    want, smax, sigma, xhat = R.add_layernorm_lens(x, res, gamma, beta, lens, R.LN_EPS)
    bound = R.layernorm_bound(want, smax, sigma, xhat, gamma, R.LN_EPS, D, has_res)
    s = torch.from_numpy(x) + torch.from_numpy(res) if has_res else torch.from_numpy(x)
    y = F.layer_norm(s, (D,), torch.from_numpy(gamma), torch.from_numpy(beta), float(f32(R.LN_EPS))).numpy()
    ratio = float((np.abs(y.astype(np.float64) - want) / bound).max())
    print(f'torch fp32 layer_norm, D = {D}: worst |err| / bound = {ratio:.3f}')
    assert ratio <= 1.0
    if offset and D >= 64:                  # E[s^2] - E[s]^2 in fp32: var ~ 1 from terms ~ 1e4, error ~ 1e4 * 2^-24 * few
        s64 = s.numpy().astype(np.float64)
        m = s.numpy().mean(-1, dtype=f32)
        v1 = (s.numpy() ** 2).mean(-1, dtype=f32) - m * m
        y1 = (s.numpy() - m[..., None]) / np.sqrt(np.maximum(v1, 0)[..., None] + f32(R.LN_EPS)) * gamma + beta
        assert float((np.abs(y1.astype(np.float64) - want) / bound).max()) > 1.0, 'the bound would pass a one-pass variance'
        assert s64.std(-1).max() < 3.0 and np.abs(s64.mean(-1)).min() > 90.0


def test_layernorm_table():
    assert (R.LN_B * R.LN_T) % 4 != 0 and len(R.LN_LENS) == R.LN_B == len(R.LN_LENS_EDGE)
    assert max(R.LN_LENS) == R.LN_T and min(R.LN_LENS) == 1
    assert min(R.LN_LENS_EDGE) == 0 and max(R.LN_LENS_EDGE) > R.LN_T
    assert min(R.LN_DIMS) < 64 and 64 in R.LN_DIMS and any(D % 64 and D > 64 for D in R.LN_DIMS)
    for D in R.LN_DIMS:
        beta = R.layernorm_inputs(D, True, False)[3]
        assert np.abs(beta).min() >= 0.5 and (beta > 0).any() and (beta < 0).any()


# ---- transpose + pad -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T,C,Tout', R.TP_SHAPES)
def test_transpose_pad_lens_equals_indexing(B, T, C, Tout):
    x = np.random.default_rng(T).standard_normal((B, T, C)).astype(f32)
    seen = set()
    for lens in R.transpose_lens_sets(B, T):
        assert len(lens) == B
        seen.update(lens)
        out = R.transpose_pad_lens(x, lens, Tout, R.PAD)
        assert out.dtype == f32 and out.shape == (B, C, Tout)
        for b in range(B):
            for t in range(Tout):
                inside = t < min(max(lens[b], 0), T)
                assert np.array_equal(out[b, :, t], x[b, t] if inside else np.full(C, f32(R.PAD)))
    assert {0, 1, T, T + 3, 31, 32, 33} <= seen and min(seen) < 0
    assert abs(R.PAD - math.log(1e-5)) < 1e-6 and R.PAD != 0.0 and float(f32(R.PAD)) == R.PAD


# ---- durations -----------------------------------------------------------------------------------------------------
def torch_item(d, L):
    """the reference's statements on ONE item of L tokens, torch CPU float32 -> (dur [Tx], frames int64 [Tx])"""
    out = torch.zeros_like(d)
    v = d[:L].clone()
    if v.long().sum() <= 0:
        torch.fill_(v, 2.)
    v[v < 0] = 0.
    out[:L] = v
    return out, (out + 0.5).long()


def torch_batch(dur, x_len):
    B, Tx = dur.shape
    outs, mel, cums, bad = [], [], [], 0
    for b in range(B):
        L = int(x_len[b])
        if L < 1 or L > Tx:
            bad, L = 1, (1 if L < 1 else Tx)
        o, r = torch_item(torch.from_numpy(dur[b]), L)
        outs.append(o.numpy())
        mel.append(int(r.sum()))
        cums.append(np.concatenate([[0], np.cumsum(r.numpy())]))
    return np.stack(outs), np.asarray(mel, dtype=np.int64), np.stack(cums).astype(np.int32), bad


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def check_against_torch(dur, x_len):
    got, mel_len, bad = R.gen_durations(dur, x_len)
    want, mel, cum, wbad = torch_batch(dur, x_len)
    assert got.dtype == f32 and mel_len.dtype == np.int64
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(mel_len, mel) and bad == wbad
    c, total = R.lr_scan(got)
    assert c.dtype == np.int32 and total.dtype == np.int32
    assert np.array_equal(c, cum) and np.array_equal(total, mel_len)
    c2, total2 = R.lr_scan(np.where(np.isnan(dur) | (dur > 1e20), f32(0), dur))          # the scan's own clamp
    r = (torch.from_numpy(np.where(np.isnan(dur) | (dur > 1e20), f32(0), dur)).clamp(min=0) + 0.5).long().numpy()
    assert np.array_equal(c2[:, 1:], np.cumsum(r, 1)) and np.array_equal(total2, r.sum(1))
    return got, mel_len, bad


@pytest.mark.parametrize('Tx', R.DUR_TX)
@pytest.mark.parametrize('in_range', [False, True])
def test_duration_table_equals_torch_per_item(Tx, in_range):
    names, dur, x_len = R.duration_table(Tx, in_range)
    got, mel_len, bad = check_against_torch(dur, x_len)
    assert bad == (0 if in_range else 1)
    assert np.all(np.isfinite(got)), 'the junk in the padding came through'


def test_durations_random_items_equal_torch():
    g = np.random.default_rng(5)
    for i in range(200):
        Tx = int(g.integers(1, 141))
        kind = i % 4
        if kind == 0:
            d = g.standard_normal(Tx) * 1.5
        elif kind == 1:
            d = g.integers(-3, 8, Tx) / 2.0                               # exactly on integers and half-integers
        elif kind == 2:
            d = np.nextafter((g.integers(0, 6, Tx) / 2.0).astype(f32), f32(-1.0))       # one ulp below them
        else:
            d = g.random(Tx) * 0.99                                       # truncated sum 0: fallback
        L = int(g.integers(-1, Tx + 3))
        check_against_torch(np.asarray(d, dtype=f32)[None], np.asarray([L]))


def test_duration_edges_are_edges():
    h, one = f32(0.49999997), f32(0.99999994)
    assert h < f32(0.5) and h + f32(0.5) == f32(1.0) and float(h) == 0.5 - 2.0 ** -25
    assert one < f32(1.0) and np.trunc(one) == 0 and np.trunc(one + f32(0.5)) == 1 and float(one) == 1 - 2.0 ** -24
    assert np.trunc(f32(0.5) + f32(0.5)) == 1 and np.trunc(f32(1.5) + f32(0.5)) == 2 and np.trunc(f32(1.5)) == 1
    assert np.signbit(f32(-0.0)) and not f32(-0.0) < 0
    assert np.trunc(f32(-0.3)) == 0 and np.trunc(f32(-0.9999)) == 0 and np.trunc(f32(-0.9999) + f32(0.5)) == 0
    assert set(R.DUR_TX) == {1, 63, 64, 65, 130}
    for Tx in R.DUR_TX:
        names, dur, x_len = R.duration_table(Tx)
        L = np.clip(x_len, 1, Tx)
        inside = np.arange(Tx)[None, :] < L[:, None]
        assert np.all(np.isfinite(dur[inside])) and np.abs(dur[inside]).max() < 10, 'nothing unspecified inside a length'
        assert np.all(~np.isfinite(dur[~inside]) | (dur[~inside] == f32(1e30)))
        assert {0, -3, Tx + 1} <= set(x_len.tolist())
        flat = set(bits(dur[inside]).tolist())
        assert set(bits(np.asarray(R.DUR_EDGES, dtype=f32)).tolist()) <= flat, 'every edge value sits inside a length'
        out, mel_len, bad = R.gen_durations(dur, x_len)
        tr = np.asarray([np.trunc(dur[b, :L[b]]).sum() for b in range(len(L))])
        fell = np.asarray([bool((out[b, :L[b]] == 2).all()) and tr[b] <= 0 for b in range(len(L))])
        assert np.array_equal(fell, tr <= 0)
        if Tx == 1:
            continue
        assert inside.sum(1).min() == 1 and (~inside).any()
        i = names.index('edges')
        assert not fell[i] and x_len[i] == Tx
        i = names.index('all 0.6')
        assert tr[i] == 0 and fell[i] and np.all(R._frames(dur[i, :L[i]]) == 1) and mel_len[i] == 2 * L[i]
        assert not fell[i - 1] and not fell[i + 1], 'the fallback item sits between two ordinary ones'
        i = names.index('truncated sum 0')
        assert tr[i] == 0 and fell[i] and (dur[i, :L[i]] < -1).any()
        i = names.index('truncated sum 1')
        assert tr[i] == 1 and not fell[i] and (dur[i, :L[i]] < -1).any() and np.all(out[i] >= 0)
        if Tx > 64:
            assert np.all(R.lr_scan(out)[0][:, 64] > 0), 'the scan carries a non-zero sum into its second chunk'


# ---- token check ---------------------------------------------------------------------------------------------------
def test_check_tokens():
    B, T, lens = R.TOK_B, R.TOK_T, R.TOK_LENS
    assert B * T > 4 * 256 and (B - 1) * T + lens[-1] - 1 >= 4 * 256, 'the last item is the last block\'s'
    idx = np.ones((B, T), dtype=np.int64)
    assert R.check_tokens(idx, lens) == 0
    idx[~R.valid_rows(lens, T)] = 0
    assert R.check_tokens(idx, lens) == 0
    idx[B - 1, lens[-1] - 1] = 0
    assert R.check_tokens(idx, lens) == 2
    idx[B - 1, lens[-1] - 1] = 1
    idx[B - 1, lens[-1]] = 0
    assert R.check_tokens(idx, lens) == 0
