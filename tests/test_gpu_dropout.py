"""GPU: the counter-based dropout mask of the kernels against its numpy restatement (tests/dropout_cpu.py), bit for bit --
ft_dropout itself, the Griffin-Lim phase draw, and every kernel that fuses the mask, each addressed directly (not
through hip.dropout), at the smallest shape that separates the index conventions a site could confuse (padded leading
dimension for the key count, item for frame).  This anchors the statistics of test_dropout_cpu.py, the dropout-on model
tests, and the older tests that rebuild their mask with hip.dropout.

ft_dropout's kept value is x / (1.0f - p) as one IEEE float32 division: it equals numpy's float32 quotient exactly at
every case below (no ulp of slack is needed or given).

p = nextafter(1, 0) = 1 - 2^-24 equals the LARGEST u, so an element with h >> 8 == 0xFFFFFF survives it (one in 2^24);
the 2^26 case looks for such elements and compares them like all others."""
import math

import numpy as np
import pytest
import torch

import dropout_cpu as D

pytestmark = pytest.mark.gpu

TOP = float(np.nextafter(np.float32(1), np.float32(0)))
PS = (0.0, 2.0 ** -24, 0.1, 0.5, 0.9, TOP)
SEEDS = [0, 1, 1 << 32, (1 << 32) + 1, (1 << 62) - 1, -1] + D.seed_stream(0, 3)     # -1: 2^64 - 1 through the wrapper's masking
BIG_SEED, BIG_N = 0x1234567890ABCDE, 1 << 26


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('n', [1, 255, 256, 257, (1 << 20) + 3])
def test_ft_dropout_bit_for_bit(n):
    """zero pattern == ~keep; dropped elements are +0.0 even where x is NaN or inf (a select, not a multiply); kept
    elements are numpy's float32 x / (1 - p) exactly"""
    from forwardtacotron_amd import hip as H
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    for j, v in enumerate((float('inf'), float('-inf'), float('nan'))):
        x[j * 7 % n::max(n // 5, 1) + j] = v                               # a few of each, spread over the blocks
    xd, xn = x.cuda(), x.numpy()
    for seed in SEEDS:
        h24 = D.hash32(seed, np.arange(n, dtype=np.uint64)) >> np.uint32(8)
        u = h24.astype(np.float32) * np.float32(2.0 ** -24)
        for p in PS:
            out = H.dropout(xd, p, seed).cpu().numpy()
            keep = u >= np.float32(p)
            with np.errstate(invalid='ignore'):
                want = np.where(keep, xn / (np.float32(1) - np.float32(p)), np.float32(0))
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(out), nan), (n, seed, p)
            assert np.array_equal(_bits(out)[~nan], _bits(want)[~nan]), (n, seed, p)    # bits: a dropped -x is +0.0, not -0.0
            assert not np.signbit(out[~keep]).any() and (out[~keep] == 0).all()


@pytest.fixture(scope='module')
def big_h24():
    return D.hash32(BIG_SEED, np.arange(BIG_N, dtype=np.uint64)) >> np.uint32(8)


@pytest.mark.parametrize('p', [0.5, 2.0 ** -24, TOP])
def test_the_boundary_u_equals_p(big_h24, p):
    """2^26 elements hold every boundary: u == 0.5 exactly, h >> 8 == 0 (the only elements p = 2^-24 drops) and
    h >> 8 == 1 (u == 2^-24 == p: kept).  They must exist, or `>` for `>=` and a rounding int -> float conversion would
    pass unseen."""
    from forwardtacotron_amd import hip as H
    at = lambda v: int((big_h24 == v).sum())
    print(f'n = 2^26: u == 0.5 at {at(1 << 23)}, h24 == 0 at {at(0)}, h24 == 1 at {at(1)}, h24 == 0xFFFFFF at {at(0xFFFFFF)}')
    if p == 0.5:
        assert at(1 << 23) >= 1
    elif p < 0.5:
        assert at(0) >= 1 and at(1) >= 1
    keep = big_h24.astype(np.float32) * np.float32(2.0 ** -24) >= np.float32(p)
    out = H.dropout(torch.ones(BIG_N, device='cuda'), p, BIG_SEED).cpu().numpy()
    want = np.where(keep, np.float32(1) / (np.float32(1) - np.float32(p)), np.float32(0))
    assert np.array_equal(_bits(out), _bits(want))


def test_host_contract():
    from forwardtacotron_amd import _lib, hip as H
    x = torch.ones(8, device='cuda')
    for p in (-0.1, 1.0, float('nan'), 1.5):
        with pytest.raises(_lib.FtError, match=r'dropout: p must be in \[0,1\)'):
            H.dropout(x, p, 1)
    out = H.dropout(torch.empty(0, device='cuda'), 0.5, 1)                  # n = 0: returns before any launch
    assert out.numel() == 0
    torch.cuda.synchronize()


def test_dropout_fn_masks_the_gradient_and_indexes_the_contiguous_copy():
    from forwardtacotron_amd.ops import DropoutFn
    g = torch.Generator().manual_seed(5)
    p, seed = 0.5, D.seed_stream(0, 1)[0]
    x = torch.randn(6, 10, generator=g).t()                                 # [10, 6], not contiguous
    w = torch.randn(6, 10, generator=g).t()
    assert not x.is_contiguous()
    mask = torch.from_numpy(D.site_mask(seed, (10, 6), p, np.float32))      # flat index of x.contiguous()
    xd = x.cuda().requires_grad_(True)
    assert not xd.is_contiguous()
    y = DropoutFn.apply(xd, p, seed)
    (y * w.cuda()).sum().backward()
    assert torch.equal(y.detach().cpu(), x * mask)                          # p = 0.5: x / 0.5 == x * 2 exactly
    assert torch.equal(xd.grad.cpu(), w * mask)
    assert 10 < int((mask == 0).sum()) < 50


@pytest.mark.parametrize('seed', [0, 1, 0x2F0E1D2C3B4A5968])
def test_the_griffin_lim_draw(seed):
    """u is keyed on (frame within the item, bin), not on the item or the packed row"""
    from forwardtacotron_amd import hip as H
    B, Tcap, Tmax, Fp, lens = 2, 11, 9, 20, [5, 9]
    S = torch.ones(B * Tcap, Fp, device='cuda')
    _, u = H.gl_init_ragged(S, torch.tensor(lens, dtype=torch.int64).cuda(), B, Tcap, Tmax, seed=seed, want_u=True)
    u = u.cpu().numpy().reshape(B, Tcap, Fp)
    want = D.u24(seed, np.arange(Tcap * Fp, dtype=np.uint64)).reshape(Tcap, Fp)       # index n * Fp + m
    for b, N in enumerate(lens):
        assert np.array_equal(_bits(u[b, :N]), _bits(want[:N])), b
    assert not np.array_equal(u[1, :5], D.u24(seed, np.arange(Tcap * Fp, 2 * Tcap * Fp, dtype=np.uint64)).reshape(Tcap, Fp)[:5])


# ---- the fused sites ----------------------------------------------------------------------------------------------------
def _padded(a, Tp):
    out = torch.zeros(*a.shape[:-1], Tp, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


@pytest.mark.parametrize('T', [7, 70])
def test_softmax_dropout_indexes_by_the_key_count(T):
    """ft_softmax_fwd / ft_softmax_bwd on [B,nh,T,Tp] buffers, Tp = T rounded up to 4 (8 and 72): the mask index is
    row * T + k, not row * Tp + k.  Key-padded columns are zero with or without the mask and are left out."""
    from forwardtacotron_amd import _lib, hip as H
    B, nh, p, seed = 2, 2, 0.5, D.seed_stream(0, 2)[1]
    Tp = (T + 3) // 4 * 4
    assert Tp != T
    g = torch.Generator().manual_seed(T)
    s = torch.randn(B, nh, T, T, generator=g, dtype=torch.float64)
    lens = [T, T - 2]
    key_pad = torch.tensor([[k >= n for k in range(T)] for n in lens])
    scale = 0.37
    mask = torch.from_numpy(D.site_mask(seed, (B, nh, T, T), p))
    valid = ~key_pad[:, None, None, :].expand(B, nh, T, T)
    P_ref = torch.softmax((s.float().double() * scale).masked_fill(~valid, float('-inf')), dim=-1)
    Pd_ref = P_ref * mask

    P = _padded(s.float(), Tp).cuda()
    Pd = torch.full_like(P, float('nan'))
    kp = key_pad.to(torch.uint8).cuda()
    _lib.call('ft_softmax_fwd', P.data_ptr(), kp.data_ptr(), B, nh, T, T, Tp, scale, Pd.data_ptr(), p, seed, H._stream())
    torch.cuda.synchronize()
    P, Pd = P.cpu(), Pd.cpu()
    assert float(P[..., T:].abs().max()) == 0 and float(Pd[..., T:].abs().max()) == 0
    assert float((P[..., :T].double() - P_ref).abs().max()) < 1e-6
    assert torch.equal((Pd[..., :T] == 0)[valid], (mask == 0)[valid])
    assert 0.3 < float((mask == 0)[valid].double().mean()) < 0.7
    assert float((Pd[..., :T].double() - Pd_ref).abs().max()) < 2e-6

    # backward: dP arrives as the gradient of the DROPPED probabilities, the kernel re-derives the mask
    gP = torch.randn(B, nh, T, T, generator=g, dtype=torch.float64).float()
    gm = gP.double() * mask
    dS_ref = scale * P_ref * (gm - (gm * P_ref).sum(-1, keepdim=True))
    dP = _padded(gP, Tp).cuda()
    Pdev = _padded(P_ref.float(), Tp).cuda()
    _lib.call('ft_softmax_bwd', Pdev.data_ptr(), dP.data_ptr(), B, nh, T, T, Tp, scale, p, seed, H._stream())
    dP = dP.cpu()
    assert float(dP[..., T:].abs().max()) == 0
    err = float((dP[..., :T].double() - dS_ref).abs().max())
    print(f'T {T}: softmax_bwd with dropout vs float64: {err:.2e} (a mask at the padded index would be O(0.1))')
    assert err < 2e-6 * max(1.0, float(dS_ref.abs().max()))


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_fused_attention_mask_with_identity_values(p):
    """ft_attn_fwd at T = hd = 64 with V the identity in every head: the output IS the dropped probability matrix,
    [b, q, h * hd + k] = dropout(P)[b, h, q, k], so its zeros are the mask over ((b * nh + h) * T + q) * T + k."""
    from forwardtacotron_amd import hip as H
    B, nh, T = 2, 2, 64
    hd, d = T, nh * T
    g = torch.Generator().manual_seed(64)
    seed = D.seed_stream(0, 3)[2]
    qkv = torch.randn(B, T, 3 * d, generator=g) * 0.7
    qkv[:, :, 2 * d:] = torch.eye(T).repeat(1, nh)[None]
    scale = 1.0 / math.sqrt(hd)
    att, _ = H.attn_fwd(qkv.cuda(), None, nh, scale, p, seed)
    got = att.cpu().reshape(B, T, nh, T).permute(0, 2, 1, 3)                # [B,nh,q,k]
    q, k = (t.bfloat16().double().reshape(B, T, nh, hd).permute(0, 2, 1, 3) for t in (qkv[..., :d], qkv[..., d:2 * d]))
    P = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
    mask = torch.from_numpy(D.site_mask(seed, (B, nh, T, T), p))
    big = P > 1e-3
    assert float(big.double().mean()) > 0.9
    assert torch.equal((got == 0)[big], (mask == 0)[big])
    assert abs(float((mask == 0).double().mean()) - p) < 0.02
    assert float((got.double() - P * mask).abs().max()) < 1e-2 * float((P * mask).max())


@pytest.mark.parametrize('rows,Dm', [(27, 16), (65, 130)])
def test_add_layernorm_with_dropout_vs_float64(rows, Dm):
    """addln_fwd's LayerNorm(x + dropout(res)) against float64 on x + site_mask * res, at test_add_layernorm's bar
    (5e-6); addln_bwd's residual gradient is zero exactly where the mask is"""
    from forwardtacotron_amd.fastpitch import addln_bwd, addln_fwd
    g = torch.Generator().manual_seed(rows + Dm)
    x, r, dy = (torch.randn(rows, Dm, generator=g) for _ in range(3))
    gamma = 1 + 0.2 * torch.randn(Dm, generator=g)
    beta = 0.1 * torch.randn(Dm, generator=g)
    p, seed = 0.5, D.seed_stream(0, 4)[3]
    mask = torch.from_numpy(D.site_mask(seed, (rows, Dm), p))
    leaves = [t.double().requires_grad_(True) for t in (x, r, gamma, beta)]
    y_ref = torch.nn.functional.layer_norm(leaves[0] + mask * leaves[1], (Dm,), leaves[2], leaves[3], 1e-5)
    (y_ref * dy.double()).sum().backward()
    y, tape = addln_fwd(x.cuda(), r.cuda(), gamma.cuda(), beta.cuda(), 1e-5, p, seed)
    dx, dres, dg, db = addln_bwd(tape, dy.cuda(), gamma.cuda(), beta.cuda())
    torch.cuda.synchronize()
    e = float((y.cpu().double() - y_ref.detach()).abs().max())
    print(f'({rows}, {Dm}): y {e:.2e}')
    assert e < 5e-6
    assert torch.equal(dres.cpu() == 0, mask == 0)
    for got, ref in zip((dx, dres, dg, db), leaves):
        assert float((got.cpu().double() - ref.grad).abs().max()) < 5e-5 * max(1.0, float(ref.grad.abs().max()))
