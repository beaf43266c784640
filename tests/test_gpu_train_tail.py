"""GPU parity of the kernels that end a train step -- MaskedL1, CrossEntropy, the gradient norm / clip record, Adam and
the skipped-step guard -- each called directly (hip.py wrappers, or _lib.call for the optimiser entry points) and
compared with a float64 formula written out here.

Bounds are derived from the arithmetic the kernels do (u = 2^-24, one fp32 rounding), not measured:
  MaskedL1 forward   each |x-t| is one rounding, the sum and the division run in double, one final rounding: 2^-22 relative
  MaskedL1 backward  inv, *g, *factor are three roundings: 2^-22 relative; masked elements and exact ties are exactly 0
  CrossEntropy loss  (logf(se)+mx) - l[tg] in fp32: 8u (max|logit| + ln K) absolute; dlogits 8u |g / count| absolute
  gradient norm      (float)sqrt(double) * pre_scale: 2^-22 relative; the coefficient adds +1e-6, a division and a product:
                     6u relative against the float64 formula
  Adam               no fixed number: the same three formulas evaluated in fp32 torch on the CPU are the yardstick, the
                     GPU may be 4x that implementation's worst absolute error per tensor (floor: one fp32 ulp of the value)

Every test prints its worst figure before it asserts (pytest -s).  Observed on the MI355X, as a fraction of the bound:
  MaskedL1 loss      0.20 at most ((1,1,1): 4.7e-8 relative; the 2.1M-element case 3.0e-8); backward inside 2^-22 throughout
  CrossEntropy       worst of loss and dlogits per shape, unit / x30 / +-1e4 logits:
                     (1,1) 0.00 0.00 0.00   (5,3) 0.09 0.10 0.00   (257,4) 0.22 0.28 0.06   (300,130) 0.23 0.45 0.10
                     (70001,2) 0.32 0.34 0.08; torch's own fp32 cross entropy on the same inputs: 0.10 (loss), 0.39 (dlogits)
  gradient norm      n = 1 2 3 4 5 7 1023 4097 2200003: 0.00 0.10 0.10 0.11 0.08 0.15 0.23 0.14 0.16; one 1e3 among 1e-3s: 0.006
Adam, worst GPU error over the yardstick's (allowed 4; the yardstick is 1.2e-7 (p), 3.4e-8 (m), 9.2e-10 (v) at n = 1027):
  step 1 / 2 / 10 / 1000, c = None   1.03 1.37 1.07 1.00          the same steps, c = 0.37   1.00 1.00 1.00 1.00
  five carried steps                 1.00                         14 decades, c = None / 0.37   1.00 1.00
  n = 1 2 3 5 6 7 1027 262147        0.86 1.00 1.00 1.00 1.03 1.00 1.00 1.00
(1.00: the GPU's worst error equals the yardstick's.)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # one fp32 rounding (relative)


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


def f32(v) -> float:
    """the value a float argument has once it went through the C ABI's `float`"""
    return float(np.float32(v))


def ulp32(ref: torch.Tensor) -> torch.Tensor:
    """one fp32 ulp at |ref| (float64 tensor), never below the smallest normal's"""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))          # |ref| = mantissa in [0.5, 1) * 2^e
    return torch.exp2((e - 24).double())


# ---------------------------------------------------------------------------------------------------
# MaskedL1
# ---------------------------------------------------------------------------------------------------
# (B, C, T) -> lens vectors; together they hold a 0, a T and a value above T for every shape, a negative one in some
L1_CASES = [
    ((1, 1, 1), [[0], [1], [5], [-3]]),
    ((3, 7, 13), [[0, 13, 20], [-1, 5, 13]]),
    ((4, 80, 65), [[0, 65, 99, 31]]),
    ((2, 1, 300), [[0, 300], [301, 150], [-2, 7]]),
    ((3, 80, 8801), [[0, 8801, 9999]]),          # 2,112,240 elements: beyond one sweep of the 1024-block grid
]


def _l1_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    t = torch.randn(*shape, generator=g)
    tie = torch.rand(*shape, generator=g) < 0.1      # exact ties: the gradient there is exactly 0
    t = torch.where(tie, x, t)
    return x, t, tie


def _l1_ref(x, t, lens):
    B, C, T = x.shape
    mask = (torch.arange(T)[None, :] < lens[:, None])[:, None, :].expand(B, C, T)
    den = float(C * lens.clamp(0, T).sum())
    s = float(((x.double() - t.double()).abs() * mask).sum())
    return s, den, mask


@pytest.mark.parametrize('shape,lens_list', L1_CASES, ids=[str(c[0]) for c in L1_CASES])
def test_masked_l1_fwd_bwd(H, shape, lens_list):
    x, t, tie = _l1_inputs(shape, sum(shape))
    xd, td = dev(x), dev(t)
    for lens_l in lens_list:
        lens = torch.tensor(lens_l, dtype=torch.int64)
        ld = dev(lens)
        s, den, mask = _l1_ref(x, t, lens)
        loss, inv = H.masked_l1_fwd(xd, td, ld)
        loss = float(loss)
        if den == 0:
            assert np.isnan(loss), (lens_l, loss)       # 0 / 0, as the float64 formula gives
        else:
            ref = s / den
            print(f'masked_l1 {shape} lens {lens_l}: |loss-ref|/ref = {abs(loss - ref) / max(ref, 1e-300):.3e}')
            assert abs(loss - ref) <= 2.0 ** -22 * abs(ref), (lens_l, loss, ref)
            assert abs(float(inv) - 1.0 / den) <= U / den
        sign = torch.sign(x.double() - t.double()) * mask
        for gout, factor in ((None, 1.0), (2.5, 1.0), (None, 0.1), (2.5, 0.1)):
            gd = None if gout is None else torch.tensor([gout], device='cuda')
            dx = H.masked_l1_bwd(xd, td, ld, inv, gd, factor).cpu()
            dead = ~mask | (x == t)
            assert bool((dx[dead] == 0).all()), 'masked elements and exact ties must get exactly 0'
            if den == 0:
                assert bool(dead.all())
                continue
            want = sign / den * (1.0 if gout is None else gout) * f32(factor)
            err = (dx.double() - want).abs()
            assert bool((err <= 2.0 ** -22 * want.abs()).all()), (lens_l, gout, factor, float(err.max()))
            assert bool((dx[~dead] != 0).all())
    assert bool(tie.any()) or x.numel() < 8


def test_masked_l1_autograd(H):
    from forwardtacotron_amd import ops
    x, t, _ = _l1_inputs((3, 7, 13), 5)
    lens = dev(torch.tensor([0, 13, 20]))
    xg = dev(x).requires_grad_(True)
    td = dev(t)
    loss = ops.masked_l1(xg, td, lens)
    (3 * loss).backward()
    l2, inv = H.masked_l1_fwd(xg.detach(), td, lens)
    assert torch.equal(loss.detach(), l2)
    direct = H.masked_l1_bwd(xg.detach(), td, lens, inv, torch.tensor([3.0], device='cuda'))
    assert torch.equal(xg.grad, direct)
    assert float(xg.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------
# CrossEntropy
# ---------------------------------------------------------------------------------------------------
CE_SHAPES = [(1, 1), (5, 3), (257, 4), (300, 130), (70001, 2)]      # the last: beyond one sweep of the 256-block grid
CE_SCALES = ['unit', 'x30', 'pm1e4']


def _ce_inputs(rows, K, scale, ignore, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, K, generator=g)
    if scale == 'x30':
        logits = logits * 30
    elif scale == 'pm1e4':           # one column at +1e4, one at -1e4: exp() of the raw logit overflows / underflows
        logits[:, 0] = 1e4
        if K > 1:
            logits[:, 1] = -1e4
    target = torch.randint(0, K, (rows,), generator=g)
    target[torch.rand(rows, generator=g) < 1 / 3] = ignore
    return logits, target


def _ce_ref(logits, target, ignore):
    """float64 F.cross_entropy; out-of-range targets count as ignored (what both kernels do)"""
    K = logits.shape[1]
    tg = torch.where((target < 0) | (target >= K), torch.full_like(target, ignore), target)
    lg = logits.double().requires_grad_(True)
    valid = tg != ignore
    loss = F.cross_entropy(lg, tg, ignore_index=ignore)
    count = int(valid.sum())
    if count:
        loss.backward()
        grad = lg.grad
    else:
        grad = torch.zeros_like(lg)
    return float(loss.detach()), grad, valid, count


def _ce_check(H, logits, target, ignore, tag):
    rows, K = logits.shape
    ref, dref, valid, count = _ce_ref(logits, target, ignore)
    bound = 8 * U * (float(logits.abs().max()) + np.log(K))
    ld, td = dev(logits), dev(target)
    loss, inv = H.cross_entropy_fwd(ld, td, ignore)
    loss = float(loss)
    if count == 0:
        assert np.isnan(loss) and np.isnan(ref), (tag, loss, ref)
        for gout in (None, 2.5):
            gd = None if gout is None else torch.tensor([gout], device='cuda')
            d = H.cross_entropy_bwd(ld, td, inv, gd, ignore)
            assert bool((d == 0).all()), tag
        return 0.0
    # the inputs must be ones on which torch's own fp32 cross entropy meets the bound: otherwise they, not the
    # kernel, are at fault
    tg32 = torch.where((target < 0) | (target >= K), torch.full_like(target, ignore), target)
    l32 = logits.clone().requires_grad_(True)
    t32 = F.cross_entropy(l32, tg32, ignore_index=ignore)
    assert abs(float(t32) - ref) <= bound, ('badly chosen inputs', tag)
    print(f'cross_entropy {tag}: |loss-ref| = {abs(loss - ref):.3e}, bound {bound:.3e}')
    assert abs(loss - ref) <= bound, (tag, loss, ref, bound)
    assert abs(float(inv) - 1.0 / count) <= U / count
    worst = abs(loss - ref) / bound
    for gout in (None, 2.5):
        gd = None if gout is None else torch.tensor([gout], device='cuda')
        d = H.cross_entropy_bwd(ld, td, inv, gd, ignore).cpu()
        assert bool((d[~valid] == 0).all()), 'ignored rows must get exactly 0'
        sc = (1.0 if gout is None else gout) / count
        err = float((d.double() - dref * (1.0 if gout is None else gout)).abs().max())
        assert err <= 8 * U * sc, (tag, gout, err, 8 * U * sc)
        worst = max(worst, err / (8 * U * sc))
    return worst


@pytest.mark.parametrize('scale', CE_SCALES)
@pytest.mark.parametrize('rows,K', CE_SHAPES)
def test_cross_entropy_fwd_bwd(H, rows, K, scale):
    worst = 0.0
    for ignore in (0, -100):
        logits, target = _ce_inputs(rows, K, scale, ignore, rows + K)
        worst = max(worst, _ce_check(H, logits, target, ignore, (rows, K, scale, ignore)))
    print(f'cross_entropy {(rows, K, scale)}: worst error / bound = {worst:.3f}')


@pytest.mark.parametrize('ignore', [0, -100])
def test_cross_entropy_all_ignored(H, ignore):
    """no row counts: the loss is NaN (0 / 0, like torch) and no logit gets a gradient"""
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(300, 5, generator=g)
    target = torch.full((300,), ignore, dtype=torch.int64)
    _ce_check(H, logits, target, ignore, ('all ignored', ignore))
    ld, td = dev(logits), dev(target)
    loss, inv = H.cross_entropy_fwd(ld, td, ignore)
    assert bool(torch.isnan(loss))
    assert bool((H.cross_entropy_bwd(ld, td, inv, None, ignore) == 0).all())


@pytest.mark.parametrize('ignore', [0, -100])
def test_cross_entropy_out_of_range_targets_are_ignored(H, ignore):
    """targets of -1 (not the ignore index) and K: neither pass reads logits[r, target]; both count the row as ignored"""
    rows, K = 257, 4
    logits, target = _ce_inputs(rows, K, 'unit', ignore, 9)
    clean = target.clone()
    target[3], target[100], target[256] = -1, K, K
    clean[3] = clean[100] = clean[256] = ignore
    _ce_check(H, logits, target, ignore, ('out of range', ignore))
    ld = dev(logits)
    a, inv_a = H.cross_entropy_fwd(ld, dev(target), ignore)
    b, inv_b = H.cross_entropy_fwd(ld, dev(clean), ignore)
    assert torch.equal(a, b) and torch.equal(inv_a, inv_b)
    da = H.cross_entropy_bwd(ld, dev(target), inv_a, None, ignore)
    assert torch.equal(da, H.cross_entropy_bwd(ld, dev(clean), inv_b, None, ignore))
    assert bool((da[[3, 100, 256]] == 0).all())


def test_cross_entropy_autograd(H):
    from forwardtacotron_amd import ops
    logits, target = _ce_inputs(300, 130, 'unit', 0, 2)
    lg = dev(logits.view(3, 100, 130)).requires_grad_(True)
    td = dev(target.view(3, 100))
    loss = ops.cross_entropy(lg, td, ignore_index=0)
    (2 * loss).backward()
    l2, inv = H.cross_entropy_fwd(lg.detach(), td, 0)
    assert torch.equal(loss.detach(), l2)
    direct = H.cross_entropy_bwd(lg.detach(), td, inv, torch.tensor([2.0], device='cuda'), 0)
    assert torch.equal(lg.grad, direct)


# ---------------------------------------------------------------------------------------------------
# gradient norm + clip coefficient
# ---------------------------------------------------------------------------------------------------
def _clip(H, L, g, max_norm, pre_scale, lane=None, record=None, ws=None, ws_bytes=None):
    if ws is None:
        ws = H.workspace(L.query('ft_grad_norm_workspace'), g.device)
    if record is None:
        record = torch.full((4,), 7.0, device=g.device)
    L.call('ft_clip_grad_norm', g.data_ptr(), g.numel(), float(max_norm), float(pre_scale),
           None if lane is None else lane.data_ptr(), record.data_ptr(), ws.data_ptr(),
           ws.numel() if ws_bytes is None else ws_bytes, H._stream())
    return record


def _check_record(rec, ref_norm, max_norm, pre_scale, tag):
    rec = rec.cpu().double()
    norm = ref_norm * pre_scale
    assert abs(float(rec[1]) - norm) <= 2.0 ** -22 * norm, (tag, float(rec[1]), norm)
    if max_norm > 0 and f32(max_norm) / (norm + 1e-6) < 1:
        want = pre_scale * f32(max_norm) / (norm + 1e-6)
        assert abs(float(rec[0]) - want) <= 6 * U * want, (tag, float(rec[0]), want)
        assert float(rec[0]) < pre_scale
    else:
        assert float(rec[0]) == pre_scale, (tag, float(rec[0]))          # no clipping: exactly pre_scale
    assert float(rec[2]) == 0 and float(rec[3]) == 0, tag
    return abs(float(rec[1]) - norm) / (2.0 ** -22 * norm)


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 7, 1023, 4097, 2_200_003])
def test_clip_grad_norm(H, L, n):
    """n & 3 = 1..3 with and without a float4 body; 2,200,003 floats is more than one sweep of the 2048-block grid"""
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen)
    ref = float(g.double().pow(2).sum().sqrt())
    gd = dev(g)
    worst = 0.0
    for pre_scale in (1.0, 0.5):
        for max_norm in (0.25 * ref * pre_scale, 4.0 * ref * pre_scale, 0.0):
            rec = _clip(H, L, gd, max_norm, pre_scale)
            worst = max(worst, _check_record(rec, ref, max_norm, pre_scale, (n, pre_scale, max_norm)))
            assert torch.equal(rec, _clip(H, L, gd, max_norm, pre_scale))         # bit-reproducible
    print(f'clip_grad_norm n={n}: worst norm error / bound = {worst:.3f}')


def test_clip_grad_norm_one_large_among_many_small(H, L):
    """1e3 among 2.2M elements of 1e-3: sum of squares 1e6 + 2.2, and 2^-22 on the norm is 0.48 on that sum.  A sum in which
    the large square meets the bulk of the small ones in fp32 loses them whole (ulp(1e6) = 2^-4 against block sums of about
    1e-3): one fp32 chain, fp32 atomics onto one word, or an fp32 reduction of the per-block partials.  It does not tell
    an fp32 accumulation inside one thread from a double one: those few addends are within the bound either way."""
    n = 2_200_003
    g = torch.full((n,), 1e-3)
    g[n // 2 + 1] = 1e3
    ref = float(g.double().pow(2).sum().sqrt())
    rec = _clip(H, L, dev(g), 1.0, 1.0)
    r = _check_record(rec, ref, 1.0, 1.0, 'one large')
    print(f'clip_grad_norm one large among small: norm error / bound = {r:.3f}')


def test_clip_grad_norm_host_refusals(H, L):
    """argument checks on the host: nothing is launched, the record stays as it was"""
    g = torch.ones(64, device='cuda')
    rec = torch.full((4,), 7.0, device='cuda')
    with pytest.raises(L.FtError):
        _clip(H, L, g[1:], 1.0, 1.0, record=rec)                  # 4 bytes past a 16-byte boundary
    with pytest.raises(L.FtError):
        _clip(H, L, g, 1.0, 1.0, record=rec, ws_bytes=L.query('ft_grad_norm_workspace') - 8)
    torch.cuda.synchronize()
    assert bool((rec == 7.0).all())


# ---------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _adam_formulas(p, g, m, v, step, c, dtype, lr=LR, b1=B1, b2=B2, eps=EPS):
    """the three formulas in `dtype` (float64: the reference; float32: the yardstick, in the kernel's operation order).
    Every scalar has the value the kernel gets: fp32 lr / betas / eps / c, and bc = 1 - float(pow(beta, step))."""
    t = lambda s: torch.tensor(f32(s), dtype=dtype)                           # noqa: E731
    one = torch.tensor(1.0, dtype=dtype)
    bc1 = torch.tensor(float(np.float32(1) - np.float32(f32(b1) ** step)), dtype=dtype)
    bc2 = torch.tensor(float(np.float32(1) - np.float32(f32(b2) ** step)), dtype=dtype)
    p, g, m, v = (a.to(dtype) for a in (p, g, m, v))
    gc = g * t(c)
    m2 = m + (gc - m) * (one - t(b1))
    v2 = v * t(b2) + (one - t(b2)) * gc * gc
    if dtype == torch.float64:
        denom = v2.sqrt() / bc2.sqrt() + t(eps)
    else:
        denom = v2.sqrt() * (one / bc2.sqrt()) + t(eps)
    p2 = p - (t(lr) / bc1) * (m2 / denom)
    return p2, m2, v2


def _adam_gpu(H, L, p, g, m, v, n, step, coef=None, lr=LR, b1=B1, b2=B2, eps=EPS):
    L.call('ft_adam_step', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps, step,
           None if coef is None else coef.data_ptr(), H._stream())


def _adam_ratio(gpu, ref64, yard32):
    """worst GPU error in units of the yardstick: per tensor the fp32 CPU implementation's worst absolute error against
    float64, per element never less than a quarter ulp (so that 4 x it is one fp32 ulp of the reference value)"""
    worst = 0.0
    for a, r, y in zip(gpu, ref64, yard32):
        e_yard = float((y.double() - r).abs().max()) if r.numel() else 0.0
        unit = torch.maximum(torch.full_like(r, e_yard), ulp32(r) / 4)
        worst = max(worst, float(((a.cpu().double() - r).abs() / unit).max()))
    return worst


def _adam_case(H, L, p, g, m, v, step, c=None, tag=''):
    n = p.numel()
    coef = None if c is None else torch.tensor([c, 1.0, 0.0, 0.0], device='cuda')
    pd, gd, md, vd = dev(p.clone()), dev(g), dev(m.clone()), dev(v.clone())
    _adam_gpu(H, L, pd, gd, md, vd, n, step, coef)
    cc = 1.0 if c is None else c
    ref = _adam_formulas(p, g, m, v, step, cc, torch.float64)
    yard = _adam_formulas(p, g, m, v, step, cc, torch.float32)
    ratio = _adam_ratio((pd, md, vd), ref, yard)
    print(f'adam {tag}: worst GPU error / yardstick = {ratio:.3f}')
    assert ratio <= 4.0, (tag, ratio)
    assert torch.equal(gd.cpu(), g)
    return ratio


def _adam_state(n, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * scale
    m = torch.randn(n, generator=gen) * 0.1 * scale
    v = torch.rand(n, generator=gen) * 0.01 * scale * scale
    return p, g, m, v


@pytest.mark.parametrize('c', [None, 0.37])
@pytest.mark.parametrize('step', [1, 2, 10, 1000])
def test_adam_one_step_from_random_state(H, L, step, c):
    p, g, m, v = _adam_state(1027, step)
    _adam_case(H, L, p, g, m, v, step, c, tag=f'step {step} c {c}')


def test_adam_five_steps_from_zero(H, L):
    """five consecutive steps, a fresh gradient each, the state carried forward in all three implementations"""
    n = 4099
    gen = torch.Generator().manual_seed(21)
    p0 = torch.randn(n, generator=gen)
    gpu = [dev(p0.clone()), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')]
    ref = [p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)]
    yard = [p0.clone(), torch.zeros(n), torch.zeros(n)]
    worst = 0.0
    for step in range(1, 6):
        g = torch.randn(n, generator=gen) * (0.1 + torch.rand(n, generator=gen))
        _adam_gpu(H, L, gpu[0], dev(g), gpu[1], gpu[2], n, step)
        ref = list(_adam_formulas(ref[0], g, ref[1], ref[2], step, 1.0, torch.float64))
        yard = list(_adam_formulas(yard[0], g, yard[1], yard[2], step, 1.0, torch.float32))
        ratio = _adam_ratio(gpu, ref, yard)
        worst = max(worst, ratio)
        assert ratio <= 4.0, (step, ratio)
    print(f'adam five steps: worst GPU error / yardstick = {worst:.3f}')
    assert float((gpu[0].cpu() != p0).float().mean()) > 0.99


@pytest.mark.parametrize('n', [1, 2, 3, 5, 6, 7, 1027, 262147])
def test_adam_tails_and_sentinels(H, L, n):
    """every scalar-tail length 1..3 with and without a float4 body; the float after each buffer stays untouched"""
    SENT = 12345.678
    p, g, m, v = _adam_state(n, n)
    bufs = []
    for a in (p, g, m, v):
        b = torch.full((n + 4,), SENT)
        b[:n] = a
        bufs.append(dev(b))
    _adam_gpu(H, L, *bufs, n, 3)
    ref = _adam_formulas(p, g, m, v, 3, 1.0, torch.float64)
    yard = _adam_formulas(p, g, m, v, 3, 1.0, torch.float32)
    ratio = _adam_ratio([bufs[0][:n], bufs[2][:n], bufs[3][:n]], ref, yard)
    print(f'adam n={n}: worst GPU error / yardstick = {ratio:.3f}')
    assert ratio <= 4.0, (n, ratio)
    for b in bufs:
        assert bool((b[n:].cpu() == torch.tensor(SENT)).all()), 'wrote past n'
    assert torch.equal(bufs[1][:n].cpu(), g)


def test_adam_gradients_from_1e_minus_12_to_1e2(H, L):
    """one buffer whose gradients span 14 decades: eps = 1e-8 decides the update of the small ones and is invisible in the
    large ones"""
    n = 4099
    gen = torch.Generator().manual_seed(5)
    mag = 10.0 ** (torch.rand(n, generator=gen) * 14 - 12)
    sgn = lambda: torch.sign(torch.randn(n, generator=gen))                   # noqa: E731
    p = torch.randn(n, generator=gen)
    g = mag * sgn() * (0.5 + torch.rand(n, generator=gen))
    m = mag * sgn() * 0.5
    v = mag * mag * 0.3
    for c in (None, 0.37):
        _adam_case(H, L, p, g, m, v, 3, c, tag=f'14 decades c {c}')
    # eps did matter for some elements and not for others
    ref = _adam_formulas(p, g, m, v, 3, 1.0, torch.float64)[0]
    noeps = _adam_formulas(p, g, m, v, 3, 1.0, torch.float64, eps=0.0)[0]
    d = (ref - noeps).abs()
    assert float(d.max()) > 1e-5 and float(d.min()) < 1e-12


def test_adam_host_refusals(H, L):
    p, g, m, v = (dev(a) for a in _adam_state(64, 0))
    before = p.clone()
    with pytest.raises(L.FtError):
        _adam_gpu(H, L, p, g, m, v, 64, 0)                        # steps count from 1
    with pytest.raises(L.FtError):
        _adam_gpu(H, L, p[1:], g, m, v, 60, 1)                    # params 4 bytes past a 16-byte boundary
    torch.cuda.synchronize()
    assert torch.equal(p, before)


# ---------------------------------------------------------------------------------------------------
# skipped step + guarded restore (remote fault lane only: the device's own fault word is never touched)
# ---------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32).cpu()


@pytest.mark.parametrize('lane0', [0.0, 1.0, float('nan')], ids=['clean', 'remote_fault', 'nan_lane'])
def test_fault_lane_skips_step_and_restores(H, L, lane0):
    H.check_rnn_status(clear=False)          # clean device: everything below is decided by the lane alone
    n = 1027
    p, g, m, v = _adam_state(n, 3)
    pd, gd, md, vd = dev(p.clone()), dev(g), dev(m.clone()), dev(v.clone())
    lane = torch.tensor([lane0, 0.0, 0.0, 0.0], device='cuda')
    ref_norm = float(g.double().pow(2).sum().sqrt())
    rec = _clip(H, L, gd, 0.25 * ref_norm, 1.0, lane=lane)
    bad = lane0 != 0.0
    if bad:
        r = rec.cpu()
        assert float(r[0]) == 0 and bool(torch.isnan(r[1])) and float(r[2]) == 2 and float(r[3]) == 0
    else:
        _check_record(rec, ref_norm, 0.25 * ref_norm, 1.0, 'clean lane')
    _adam_gpu(H, L, pd, gd, md, vd, n, 2, rec)
    if bad:
        for a, b in ((pd, p), (md, m), (vd, v)):
            assert torch.equal(_bits(a), b.view(torch.int32)), 'a skipped step must leave p, m, v bit-identical'
    else:
        c = float(rec[0])
        ref = _adam_formulas(p, g, m, v, 2, c, torch.float64)
        yard = _adam_formulas(p, g, m, v, 2, c, torch.float32)
        assert _adam_ratio((pd, md, vd), ref, yard) <= 4.0
        assert float((pd.cpu() != p).float().mean()) > 0.99, 'a clean lane must let the update through'
    gen = torch.Generator().manual_seed(8)
    for nwords in (1, 255, 65537):           # 65537 words: beyond one sweep of the 256-block grid
        snap = torch.randint(-2 ** 31, 2 ** 31 - 1, (nwords + 1,), generator=gen, dtype=torch.int64).to(torch.int32)
        cur = torch.randint(-2 ** 31, 2 ** 31 - 1, (nwords + 1,), generator=gen, dtype=torch.int64).to(torch.int32)
        dst, sd = dev(cur.clone()), dev(snap)
        L.call('ft_guarded_restore', dst.data_ptr(), sd.data_ptr(), nwords, rec.data_ptr(), H._stream())
        want = cur.clone()
        if bad:
            want[:nwords] = snap[:nwords]
        assert torch.equal(dst.cpu(), want), (nwords, bad)         # (word nwords is never written)
        assert torch.equal(sd.cpu(), snap)
    H.check_rnn_status(clear=False)


def test_fault_lane_set_on_clean_device(H, L):
    H.check_rnn_status(clear=False)
    lane = torch.full((4,), 7.0, device='cuda')
    L.call('ft_fault_lane_set', lane.data_ptr(), H._stream())
    assert bool((lane.cpu() == 0).all())
    with pytest.raises(L.FtError):
        L.call('ft_fault_lane_set', lane[1:].data_ptr(), H._stream())
