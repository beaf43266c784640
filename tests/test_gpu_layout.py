"""GPU parity of the small data-movement kernels between the big ones: transpose_pad, concat / slice of feature columns,
the pitch / energy conditioning, fill_padded / mask_rows, copy_segments, the embedding kernels and the LengthRegulator
paths no other test reaches (time-major expand / backward, the wide batch-major backward).

These kernels move or select fp32 values, so the comparisons are torch.equal against plain torch indexing.  The
exceptions and their bounds (u = 2^-24, one fp32 rounding):
  cond_add_fwd        at most 8 fp32 operations per output: 8u (|x| + |sp| sum|terms_p| + |se| sum|terms_e|) per element
  lr_bwd / lr_bwd_tm  a sum of n frames in frame order: n u sum|terms| per element
  embedding_bwd, CondAddFn weight gradients: TN GEMMs in the fp32 mode, the 2e-6 relative bar test_linear_fwd_bwd sets
                      for linear_bwd_weight

Observed on the MI355X: cond_add_fwd at most 0.29 of its bound ((3,17,16) and (4,9,33)); lr_bwd_tm 0.13 / 0.50 / 0.51 /
0.55 for the four shapes, lr_bwd 0.50 at C = 1024 and 1028, both bit-equal to C = 1020 on the shared columns;
CondAddFn weight and bias gradients at most 2.1e-7, embedding_bwd 1.3e-7 (C = 10) and 1.1e-7 (C = 256) relative.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = -11.5


@pytest.fixture(scope='module')
def H():
    from forwardtacotron_amd import hip
    assert torch.cuda.is_available()
    return hip


@pytest.fixture(scope='module')
def L():
    from forwardtacotron_amd import _lib
    return _lib


def dev(t):
    return t.cuda().contiguous()


# ---------------------------------------------------------------------------------------------------
# transpose_pad
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', [PAD, 0.0])
@pytest.mark.parametrize('B,T,C,Tout', [(1, 1, 1, 1), (2, 31, 33, 31), (3, 33, 31, 40), (2, 65, 80, 64), (2, 64, 64, 97)])
def test_transpose_pad(H, B, T, C, Tout, pad):
    g = torch.Generator().manual_seed(T * 100 + C)
    x = torch.randn(B, T, C, generator=g)
    n = min(T, Tout)
    ref = torch.full((B, C, Tout), pad)
    ref[:, :, :n] = x[:, :n].transpose(1, 2)
    assert torch.equal(H.transpose_pad_fwd(dev(x), Tout, pad).cpu(), ref)
    dout = torch.randn(B, C, Tout, generator=g)
    dref = torch.zeros(B, T, C)                   # the adjoint: frames the forward dropped or padded get no gradient
    dref[:, :n] = dout[:, :, :n].transpose(1, 2)
    assert torch.equal(H.transpose_pad_bwd(dev(dout), T).cpu(), dref)


def test_transpose2d(H):
    g = torch.Generator().manual_seed(2)
    for R, C in ((1, 1), (33, 65), (64, 32)):
        w = torch.randn(R, C, generator=g)
        assert torch.equal(H.transpose2d(dev(w)).cpu(), w.t().contiguous())


# ---------------------------------------------------------------------------------------------------
# concat_cols / slice_cols
# ---------------------------------------------------------------------------------------------------
CONCAT_CASES = [(3, 5, 7, 0, 0), (2, 9, 4, 3, 5), (5, 3, 16, 1, 0), (4, 6, 6, 0, 8)]


def _concat_inputs(B, T, Ca, Cb, S):
    g = torch.Generator().manual_seed(B * 10 + T)
    a = torch.randn(B, T, Ca, generator=g)
    b2 = torch.randn(B, T, Cb, generator=g) if Cb else None
    semb = torch.randn(B, S, generator=g) if S else None
    parts = [a] + ([b2] if Cb else []) + ([semb[:, None, :].expand(B, T, S)] if S else [])
    return a, b2, semb, torch.cat(parts, dim=2), g


@pytest.mark.parametrize('a_tm', [False, True], ids=['a_batch_major', 'a_time_major'])
@pytest.mark.parametrize('B,T,Ca,Cb,S', CONCAT_CASES)
def test_concat_cols(H, B, T, Ca, Cb, S, a_tm):
    from forwardtacotron_amd import ops
    a, b2, semb, ref, g = _concat_inputs(B, T, Ca, Cb, S)
    a_in = a.transpose(0, 1).contiguous() if a_tm else a
    ad = dev(a_in)
    b2d = dev(b2) if b2 is not None else None
    sd = dev(semb) if semb is not None else None
    assert torch.equal(H.concat_cols(ad, b2d, sd, B, T, a_tm).cpu(), ref)
    ag = ad.clone().requires_grad_(True)
    bg = b2d.clone().requires_grad_(True) if b2d is not None else None
    out = ops.ConcatColsFn.apply(ag, bg, sd, B, T, a_tm)
    assert torch.equal(out.detach().cpu(), ref)
    dout = torch.randn(B, T, Ca + Cb + S, generator=g)
    out.backward(dev(dout))
    da = dout[..., :Ca]
    assert torch.equal(ag.grad.cpu(), da.transpose(0, 1).contiguous() if a_tm else da.contiguous())
    if bg is not None:
        assert torch.equal(bg.grad.cpu(), dout[..., Ca:Ca + Cb].contiguous())


@pytest.mark.parametrize('dst_tm', [False, True], ids=['dst_batch_major', 'dst_time_major'])
@pytest.mark.parametrize('B,T,Ca,Cb,S', CONCAT_CASES)
def test_slice_cols(H, B, T, Ca, Cb, S, dst_tm):
    g = torch.Generator().manual_seed(B + T)
    for col0, C, extra in ((3, Ca, 2), (1, max(Cb + S, 1), 5)):         # col0 > 0 and ld > col0 + C
        ld = col0 + C + extra
        src = torch.randn(B, T, ld, generator=g)
        ref = src[..., col0:col0 + C]
        ref = ref.transpose(0, 1).contiguous() if dst_tm else ref.contiguous()
        assert torch.equal(H.slice_cols(dev(src), col0, C, dst_time_major=dst_tm).cpu(), ref)


# ---------------------------------------------------------------------------------------------------
# pitch / energy conditioning
# ---------------------------------------------------------------------------------------------------
COND_CASES = [(1, 1, 3), (2, 2, 5), (3, 17, 16), (4, 9, 33)]
SP = 0.7


def _cond_inputs(B, T, C):
    g = torch.Generator().manual_seed(B * 100 + T * 10 + C)
    r = lambda *s: torch.randn(*s, generator=g)                           # noqa: E731
    return dict(x=r(B, T, C), pitch=r(B, T), energy=r(B, T), wp=r(C, 1, 3), bp=r(C), we=r(C, 1, 3), be=r(C)), g


def _cond_ref(d, sp, se):
    """float64 conv1d(k=3, padding=1) of pitch and energy -> ([B,T,C] value, [B,T,C] sum of |terms|)"""
    def proj(sig, w, b):
        return F.conv1d(sig[:, None, :], w, b, padding=1).transpose(1, 2)
    D = {k: v.double() for k, v in d.items()}
    val = D['x'] + sp * proj(D['pitch'], D['wp'], D['bp']) + se * proj(D['energy'], D['we'], D['be'])
    mag = (D['x'].abs() + abs(sp) * proj(D['pitch'].abs(), D['wp'].abs(), D['bp'].abs())
           + abs(se) * proj(D['energy'].abs(), D['we'].abs(), D['be'].abs()))
    return val, mag


@pytest.mark.parametrize('se', [0.0, 1.0])
@pytest.mark.parametrize('x_tm', [False, True], ids=['x_batch_major', 'x_time_major'])
@pytest.mark.parametrize('B,T,C', COND_CASES)
def test_cond_add_fwd(H, B, T, C, x_tm, se):
    d, _ = _cond_inputs(B, T, C)
    sp32, se32 = float(np.float32(SP)), float(np.float32(se))
    val, mag = _cond_ref(d, sp32, se32)
    x_in = d['x'].transpose(0, 1).contiguous() if x_tm else d['x']
    out = H.cond_add_fwd(dev(x_in), dev(d['pitch']), dev(d['energy']), dev(d['wp']), dev(d['bp']), dev(d['we']),
                         dev(d['be']), SP, se, x_tm).cpu()
    assert tuple(out.shape) == (B, T, C)
    ratio = float(((out.double() - val).abs() / (8 * U * mag)).max())
    print(f'cond_add {(B, T, C)} x_tm {x_tm} se {se}: worst error / bound = {ratio:.3f}')
    assert ratio <= 1.0


@pytest.mark.parametrize('B,T,C', COND_CASES)
def test_cond_taps(H, B, T, C):
    d, _ = _cond_inputs(B, T, C)
    p, e = d['pitch'], d['energy']
    ref = torch.zeros(B, T, 8)
    for o, s in ((0, p), (4, e)):
        ref[:, 1:, o] = s[:, :-1]                 # the tap at t-1: 0 at t = 0
        ref[:, :, o + 1] = s
        ref[:, :-1, o + 2] = s[:, 1:]             # the tap at t+1: 0 at t = T-1
        ref[:, :, o + 3] = 1.0
    assert torch.equal(H.cond_taps(dev(p), dev(e)).cpu(), ref)


@pytest.mark.parametrize('se', [0.0, 1.0])
@pytest.mark.parametrize('x_tm', [False, True], ids=['x_batch_major', 'x_time_major'])
@pytest.mark.parametrize('B,T,C', COND_CASES)
def test_cond_add_autograd(H, B, T, C, x_tm, se):
    from forwardtacotron_amd import ops
    d, g = _cond_inputs(B, T, C)
    sp32, se32 = float(np.float32(SP)), float(np.float32(se))
    dout = torch.randn(B, T, C, generator=g)
    leaves = {k: v.double().requires_grad_(True) for k, v in d.items() if k in ('wp', 'bp', 'we', 'be')}
    val, _ = _cond_ref({**d, **leaves}, sp32, se32)
    (val * dout.double()).sum().backward()
    x_in = d['x'].transpose(0, 1).contiguous() if x_tm else d['x']
    xg = dev(x_in).requires_grad_(True)
    P = {k: dev(d[k]).requires_grad_(True) for k in leaves}
    old = H.set_gemm_precision('fp32')
    try:
        out = ops.CondAddFn.apply(xg, dev(d['pitch']), dev(d['energy']), P['wp'], P['bp'], P['we'], P['be'], SP, se, x_tm)
        out.backward(dev(dout))
    finally:
        H.set_gemm_precision(old)
    assert torch.equal(xg.grad.cpu(), dout.transpose(0, 1).contiguous() if x_tm else dout)
    for k in leaves:
        assert P[k].grad.shape == d[k].shape
        e = rel_err(P[k].grad, leaves[k].grad)
        print(f'cond_add {(B, T, C)} d{k}: rel err {e:.3e}')
        assert e < 2e-6, (k, e)


# ---------------------------------------------------------------------------------------------------
# fill_padded / mask_rows
# ---------------------------------------------------------------------------------------------------
# (T, B, C) -> lens vectors (None: pure layout change); with a 0 and a value above T
FILL_CASES = [((1, 1, 1), [None, [0], [1], [3]]),
              ((7, 3, 5), [None, [0, 7, 9], [3, 1, 6]]),
              ((33, 4, 16), [None, [0, 33, 40, 17]])]


@pytest.mark.parametrize('shape,lens_list', FILL_CASES, ids=[str(c[0]) for c in FILL_CASES])
def test_fill_padded_and_mask_rows(H, shape, lens_list):
    T, B, C = shape
    g = torch.Generator().manual_seed(T + B + C)
    raw = torch.randn(T, B, C, generator=g)
    bm = raw.transpose(0, 1).contiguous()
    rd, bd = dev(raw), dev(bm)
    for lens_l in lens_list:
        if lens_l is None:
            assert torch.equal(H.fill_padded(rd, None, PAD).cpu(), bm)
            continue
        lens = torch.tensor(lens_l, dtype=torch.int64)
        keep = (torch.arange(T)[None, :] < lens[:, None])[:, :, None].expand(B, T, C)
        assert torch.equal(H.fill_padded(rd, dev(lens), PAD).cpu(), torch.where(keep, bm, torch.tensor(PAD))), lens_l
        assert torch.equal(H.mask_rows(bd, dev(lens)).cpu(), torch.where(keep, bm, torch.tensor(0.0))), lens_l


def test_bt_transpose(H):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 7, 5, generator=g)
    tm = x.transpose(0, 1).contiguous()
    assert torch.equal(H.bt_transpose(dev(x), True).cpu(), tm)
    assert torch.equal(H.bt_transpose(dev(tm), False).cpu(), x)


# ---------------------------------------------------------------------------------------------------
# copy_segments
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('npairs', [1, 64, 130])
def test_copy_segments(H, npairs):
    """the wrapper chunks by 64 pairs; one workgroup strides over a segment 256 floats at a time"""
    GUARD = -777.25
    small = [0, 1, 255, 256, 257, 3, 1000]
    lens = [100_003] + [small[i % len(small)] for i in range(npairs - 1)]
    lens = lens[::-1] if npairs > 1 else lens         # the long one in the last (partial) chunk
    g = torch.Generator().manual_seed(npairs)
    src_all = dev(torch.randn(sum(lens), generator=g))
    dst_all = torch.full((sum(lens) + npairs + 1,), GUARD, device='cuda')
    srcs, dsts, so, do = [], [], 0, 1
    for n in lens:
        srcs.append(src_all[so:so + n])
        dsts.append(dst_all[do:do + n])
        so += n
        do += n + 1                                   # one guard float between destinations (and one in front)
    H.copy_segments(srcs, dsts)
    got = dst_all.cpu()
    ref = torch.full_like(got, GUARD)
    so, do = 0, 1
    sc = src_all.cpu()
    for n in lens:
        ref[do:do + n] = sc[so:so + n]
        so += n
        do += n + 1
    assert torch.equal(got, ref)


def test_copy_segments_size_mismatch(H, L):
    a, b = torch.ones(5, device='cuda'), torch.zeros(6, device='cuda')
    with pytest.raises(L.FtError):
        H.copy_segments([a], [b])
    torch.cuda.synchronize()
    assert bool((b == 0).all())


# ---------------------------------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------------------------------
def test_embedding_fwd_index_errors(H):
    V, C = 135, 10
    g = torch.Generator().manual_seed(6)
    w = torch.randn(V, C, generator=g)
    idx = torch.randint(0, V, (4, 25), generator=g)
    H.check_index_errors('cuda')                  # a flag an earlier test left set is reported here, not swallowed
    out = H.embedding_fwd(dev(idx), dev(w))
    assert torch.equal(out.cpu(), w[idx])
    H.check_index_errors('cuda')                  # in range: clean
    bad = idx.clone()
    bad[0, 3], bad[2, 24] = -1, V
    out = H.embedding_fwd(dev(bad), dev(w)).cpu()
    ref = w[bad.clamp(0, V - 1)]
    ref[0, 3] = 0
    ref[2, 24] = 0
    assert torch.equal(out, ref)
    with pytest.raises(IndexError):
        H.check_index_errors('cuda')
    H.check_index_errors('cuda')                  # raised once, then clean


def test_onehot(H):
    V = 135
    g = torch.Generator().manual_seed(7)
    idx = torch.randint(0, V, (700,), generator=g)
    assert torch.equal(H.onehot(dev(idx), V).cpu(), F.one_hot(idx, V).float())


@pytest.mark.parametrize('C', [10, 256])
def test_embedding_bwd(H, C):
    V, rows = 135, 700
    g = torch.Generator().manual_seed(C)
    used = torch.randperm(V, generator=g)[:20]                    # heavy repeats; 115 ids never occur
    idx = used[torch.randint(0, 20, (rows,), generator=g)]
    dout = torch.randn(rows, C, generator=g)
    ref = torch.zeros(V, C, dtype=torch.float64).index_add_(0, idx, dout.double())
    idxd, dd = dev(idx), dev(dout)
    old = H.set_gemm_precision('fp32')
    try:
        dw = H.embedding_bwd(idxd, dd, V)
        cache = {}
        dw2 = H.embedding_bwd(idxd, dd, V, onehot_cache=cache)
        dw3 = H.embedding_bwd(idxd, dd, V, onehot_cache=cache)    # this one reuses the cached one-hot matrix
    finally:
        H.set_gemm_precision(old)
    e = rel_err(dw, ref)
    print(f'embedding_bwd C={C}: rel err {e:.3e}')
    assert e < 2e-6
    unused = torch.ones(V, dtype=torch.bool)
    unused[used] = False
    assert int(unused.sum()) == V - 20 and bool((dw.cpu()[unused] == 0).all())
    assert len(cache) == 1
    assert torch.equal(dw2, dw) and torch.equal(dw3, dw)


# ---------------------------------------------------------------------------------------------------
# LengthRegulator: time-major expand / backward, wide batch-major backward
# ---------------------------------------------------------------------------------------------------
def _durations(B, Tx, Tm, g):
    """durations with zeros and a negative value; item 0 has more than Tm frames (the clamp runs), the last item of a
    batch fewer than Tm (padding rows exist).  Fractions stay clear of .5, so (dur + 0.5).long() is not a rounding question."""
    r = torch.randint(0, 4, (B, Tx), generator=g)
    r[0] += Tm // Tx + 2                                          # total of item 0 > Tm
    if B > 1:
        last = torch.randint(0, 2, (Tx,), generator=g)
        last[0] = 1 if Tm > 1 else 0
        while int(last.sum()) >= Tm:
            last[int(last.nonzero()[-1])] = 0
        r[B - 1] = last
    if Tx >= 3:
        r[0, 1] = 0
    dur = r.float() + (torch.rand(B, Tx, generator=g) * 0.8 - 0.4)      # (zeros with a negative fraction are < 0 too)
    if Tx >= 3:
        dur[0, 1] = -1.3                                          # negative: clamped to 0 in place
    return dur, r


def _lr_setup(H, B, Tx, C, Tm, seed):
    g = torch.Generator().manual_seed(seed)
    dur, r = _durations(B, Tx, Tm, g)
    durd = dev(dur)
    cum, total = H.lr_scan(durd)
    cum_ref = torch.cat([torch.zeros(B, 1, dtype=torch.int64), r.cumsum(1)], dim=1)
    assert torch.equal(cum.cpu().long(), cum_ref) and torch.equal(total.cpu().long(), cum_ref[:, -1])
    assert torch.equal(durd.cpu(), dur.clamp_min(0))
    assert int(cum_ref[0, -1]) > Tm
    # src[b][t]: the token frame t repeats, -1 beyond the item's frames
    src = torch.full((B, Tm), -1, dtype=torch.int64)
    for b in range(B):
        toks = torch.repeat_interleave(torch.arange(Tx), r[b])[:Tm]
        src[b, :toks.numel()] = toks
    return g, cum, cum_ref, src


LR_TM_CASES = [(1, 1, 4, 3), (3, 7, 8, 17), (2, 65, 260, 50), (4, 5, 6, 9)]     # the last: C % 4 != 0, the scalar path


@pytest.mark.parametrize('with_pad', [False, True], ids=['zeros', 'pad_row'])
@pytest.mark.parametrize('B,Tx,C,Tm', LR_TM_CASES)
def test_lr_expand_tm(H, B, Tx, C, Tm, with_pad):
    g, cum, _, src = _lr_setup(H, B, Tx, C, Tm, B + Tx + C)
    x = torch.randn(B, Tx, C, generator=g)
    pad_row = torch.randn(C, generator=g) if with_pad else None
    y = H.lr_expand_tm(dev(x), cum, Tm, dev(pad_row) if with_pad else None).cpu()
    assert tuple(y.shape) == (Tm, B, C)
    fill = pad_row if with_pad else torch.zeros(C)
    ref = torch.empty(B, Tm, C)
    for b in range(B):
        ref[b] = torch.where((src[b] >= 0)[:, None], x[b, src[b].clamp_min(0)], fill[None, :])
    assert torch.equal(y, ref.transpose(0, 1).contiguous())
    if B > 1:
        assert bool((src < 0).any())


def _lr_bwd_ref(dy_bm, src, Tx):
    """dy_bm [B,Tm,C] -> float64 (dx [B,Tx,C], tail [B,C], |.| sums of both, frame counts of both)"""
    B, Tm, C = dy_bm.shape
    d = dy_bm.double()
    dx, ax = torch.zeros(B, Tx, C, dtype=torch.float64), torch.zeros(B, Tx, C, dtype=torch.float64)
    tail, at = torch.zeros(B, C, dtype=torch.float64), torch.zeros(B, C, dtype=torch.float64)
    nx, nt = torch.zeros(B, Tx, 1, dtype=torch.float64), torch.zeros(B, 1, dtype=torch.float64)
    for b in range(B):
        on = src[b] >= 0
        dx[b].index_add_(0, src[b][on], d[b][on])
        ax[b].index_add_(0, src[b][on], d[b][on].abs())
        nx[b].index_add_(0, src[b][on], torch.ones(int(on.sum()), 1, dtype=torch.float64))
        tail[b] = d[b][~on].sum(0)
        at[b] = d[b][~on].abs().sum(0)
        nt[b] = float((~on).sum())
    return dx, tail, ax, at, nx, nt


def _check_sum(got, ref, mag, n, tag):
    err = (got.cpu().double() - ref).abs()
    bound = n * U * mag
    assert bool((err <= bound).all()), (tag, float((err - bound).max()))
    assert bool((got.cpu()[(n == 0).expand_as(ref)] == 0).all()), tag
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize('B,Tx,C,Tm', [(1, 1, 4, 3), (3, 7, 8, 17), (2, 65, 260, 50), (3, 7, 516, 17)])
def test_lr_bwd_tm(H, B, Tx, C, Tm):
    """C = 260 / 516: 2 / 3 column chunks of 256, the last one partial"""
    g, cum, _, src = _lr_setup(H, B, Tx, C, Tm, B + Tx + C)
    dy = torch.randn(Tm, B, C, generator=g)
    dx, rows = H.lr_bwd_tm(dev(dy), cum, Tx)
    assert tuple(dx.shape) == (B, Tx, C) and tuple(rows.shape) == (B * Tx + B, C)
    assert rows.data_ptr() == dx.data_ptr() and torch.equal(rows[:B * Tx].view(B, Tx, C), dx)
    rdx, rtail, ax, at, nx, nt = _lr_bwd_ref(dy.transpose(0, 1), src, Tx)
    a = _check_sum(dx, rdx, ax, nx, 'dx')
    b = _check_sum(rows[B * Tx:], rtail, at, nt, 'tail')
    print(f'lr_bwd_tm {(B, Tx, C, Tm)}: worst error / bound = {max(a, b):.3f}')
    assert float(nx.max()) > 1


def test_lr_bwd_tm_needs_16_byte_rows(H, L):
    g, cum, _, _ = _lr_setup(H, 4, 5, 6, 9, 1)
    with pytest.raises(L.FtError):
        H.lr_bwd_tm(dev(torch.randn(9, 4, 6, generator=g)), cum, 5)


def test_lr_bwd_wide_rows(H):
    """batch-major lr_bwd with C % 4 == 0 and C >= 1024 takes the one-wave-per-256-columns kernel, C = 1020 the
    one-wave-per-row kernel.  Both add a token's frames in frame order, so they agree bit for bit on the shared columns."""
    B, Tx, Tm = 3, 7, 17
    g, cum, _, src = _lr_setup(H, B, Tx, 1028, Tm, 11)
    dy = torch.randn(B, Tm, 1028, generator=g)
    narrow = H.lr_bwd(dev(dy[..., :1020]), cum, Tx).cpu()
    rdx, _, ax, _, nx, _ = _lr_bwd_ref(dy, src, Tx)
    _check_sum(narrow, rdx[..., :1020], ax[..., :1020], nx, 'C=1020')
    for C in (1024, 1028):
        dx = H.lr_bwd(dev(dy[..., :C]), cum, Tx)
        r = _check_sum(dx, rdx[..., :C], ax[..., :C], nx, f'C={C}')
        print(f'lr_bwd C={C}: worst error / bound = {r:.3f}')
        assert torch.equal(dx.cpu()[..., :1020], narrow), C
