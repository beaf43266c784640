"""GPU: the kernels of csrc/ft_taco_train.hip, called through the C ABI, against float64 autograd through
tests/taco_step_cpu.py.

ft_taco_attend_bwd: operands randn * 0.7, cotangent dhist randn; the float64 reference is autograd of
sum(hist * dhist) through taco_step_cpu.attend.  The entry's operands hist and attn are that float64 forward's own,
rounded to float32, NOT what ft_taco_attend writes on the device.  Reason, measured: at randn * 0.7 the recurrence is
chaotic (|dP|inf grows from 1.7 at S = 1 to 2.7e4 at Tx 5, S 7), so a gradient's distance from float64 is the distance
of the FORWARD state it was taken at and nothing else.  Measured on an MI355X and its host, max error against float64
relative to each array's scale, range over dep, dP, dcw, dL, dv:
    (B, Tx, S)                                       (1, 5, 7)          (3, 33, 7)         (17, 70, 7)
    stock float32 forward + stock float32 backward   5.9e-4 .. 8.1e-4   8.5e-2 .. 2.5e-1   4.2 .. 10.3
    stock float32 forward + float64 backward         5.8e-4 .. 8.0e-4   8.5e-2 .. 2.5e-1   4.2 .. 10.3   (the same)
    ft_taco_attend + float64 backward                2.3e-3 .. 3.2e-3   7.1e-2 .. 1.7e-1   15 .. 37
    ft_taco_attend + ft_taco_attend_bwd              2.3e-3 .. 3.2e-3   7.1e-2 .. 1.7e-1   15 .. 37      (the same)
    float64 forward (rounded) + ft_taco_attend_bwd   2.4e-6 .. 2.6e-5   3.3e-6 .. 6.5e-6   4.5e-6 .. 1.2e-5
(the stock rows come out up to 6 x different on another host: 3.5e-3 .. 4.9e-3 for the first case.)
The first version of this test took hist and attn from ft_taco_attend; B 1, Tx 5, S 7 then sat at 0.986 .. 1.004 of the
bound on all twelve outputs alike (dcw 23.70 against 23.62): it measured by how many stock-float32 errors the forward
kernel's trajectory -- hardware tanh, its own summation order; tests/test_gpu_taco_kernels.py holds that kernel to its
own bounds -- had drifted, times an amplification that differs from host to host, and nothing about the kernels under
test here.  With the reference trajectory as input the same bound, max(4 e_stock, 1e-4 |x64|inf), measures
ft_taco_attend_bwd itself.  The chain ft_taco_attend -> ft_taco_attend_bwd is still run in every case and its figures
are printed beside the asserted ones (reproducibility and finiteness are asserted on it too);
tests/test_gpu_tacotron_train.py asserts the chain at the model's own weights, where it is well conditioned.
ft_taco_lstm_zone_fwd / _bwd: taco_step_cpu.lstm_cell plus the zoneout mix, with the mask rebuilt on the host
(tests/dropout_cpu.py).

Bound (the project's, tests/test_gpu_full_parity.py:213-218): an array passes when its max error against float64 is at
most max(4 * e_stock, 1e-4 * |x64|inf), e_stock being the error of the same restatement run by stock torch in float32 on
the host, |x64|inf the array's OWN scale -- an all-zero gradient fails wherever the true one is not zero.  Every figure
is printed (-s).  Workspaces start as 0xFF bytes (NaN), outputs as NaN, w_ih carries NaN in the columns the attention
must not read.  Every call is made twice: the second result must equal the first bit for bit."""
import numpy as np
import pytest
import torch

import dropout_cpu
import taco_step_cpu as K
from forwardtacotron_amd import _lib
from forwardtacotron_amd import hip as H
from forwardtacotron_amd import taco_ops
from poison import poison

pytestmark = pytest.mark.gpu

D = 256
NAN = float('nan')
ATT_KEYS = ('ep', 'epq', 'P', 'w_ih', 'w_hh', 'b_hh', 'W', 'bW', 'cw', 'L', 'bL', 'v')
ATT_GRADS = dict(dep='ep', depq='epq', dP='P', dw_ih_ctx='w_ih', dw_hh='w_hh', db_hh='b_hh', dW='W', dbW='bW',
                 dcw='cw', dL='L', dbL='bL', dv='v')


def _poisoned_ws(nbytes):
    assert nbytes > 0
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device='cuda')


def _same_bits(a, b):
    """bitwise equality (NaN equals the same NaN)"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(what, got, r64, r32, enforce=True):
    """got / r64 / r32: dicts of arrays; prints error, stock error, scale and error / bound of each; asserts the bound
    (enforce=False: figures only, finiteness is still asserted)"""
    bad = []
    for k, ref in r64.items():
        g = got[k].detach().double().cpu()
        assert g.shape == ref.shape, (what, k, g.shape, ref.shape)
        assert not enforce or torch.isfinite(g).all(), (what, k)
        scale = float(ref.abs().max())
        err = float((g - ref).abs().max())
        e32 = float((r32[k].double() - ref).abs().max())
        bound = max(4 * e32, 1e-4 * scale)
        print('%s %-9s |x64|inf %.2e  stock fp32 %.2e  gpu %.2e  gpu / bound %s'
              % (what, k, scale, e32, err, '%.3f' % (err / bound) if bound > 0 else ('0/0' if err == 0 else 'inf')))
        if err > bound:
            bad.append((k, err, bound))
    assert not (bad and enforce), (what, bad)


# ---- ft_taco_attend_bwd ----------------------------------------------------------------------------------------------
def _att_operands(B, Tx, S):
    g = torch.Generator().manual_seed(1000003 * B + 1031 * Tx + S)
    n = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32) * 0.7
    o = dict(ep=n(B, Tx, D), epq=n(B, Tx, D), P=n(S, B, 3 * D), w_ih=n(3 * D, D), w_hh=n(3 * D, D), b_hh=n(3 * D),
             W=n(D, D), bW=n(D), cw=n(32, 2, 31), L=n(D, 32), bL=n(D), v=n(D))
    dhist = torch.randn(S, B, 2 * D, generator=g, dtype=torch.float32)
    return o, dhist


def _att_reference(o, dhist, dt):
    """-> (gradients by output name, hist [S,B,512], attn [B,S,Tx]) of the restatement in dt"""
    leaves = {k: o[k].to(dt).requires_grad_(True) for k in ATT_KEYS}
    attn, hist = K.attend(*(leaves[k] for k in ATT_KEYS))
    (hist * dhist.to(dt)).sum().backward()
    return {name: leaves[k].grad.detach() for name, k in ATT_GRADS.items()}, hist.detach(), attn.detach()


def _att_gpu(o, dhist, hist64, attn64, ld=384):
    """-> (ft_taco_attend_bwd on the float64 trajectory rounded to float32, the same on ft_taco_attend's own outputs)"""
    B, Tx = o['ep'].shape[:2]
    S = o['P'].shape[0]
    dev = {k: o[k].contiguous().cuda() for k in ATT_KEYS if k != 'w_ih'}
    w_ih = torch.full((3 * D, ld), NAN, device='cuda')
    w_ih[:, :D] = o['w_ih'].cuda()
    attn = torch.full((B, S, Tx), NAN, device='cuda')
    hist = torch.full((S, B, 2 * D), NAN, device='cuda')
    ws = _poisoned_ws(_lib.query('ft_taco_attend_workspace', B, Tx))
    _lib.call('ft_taco_attend', dev['ep'].data_ptr(), dev['epq'].data_ptr(), dev['P'].data_ptr(), w_ih.data_ptr(), ld,
              dev['w_hh'].data_ptr(), dev['b_hh'].data_ptr(), dev['W'].data_ptr(), dev['bW'].data_ptr(),
              dev['cw'].data_ptr(), dev['L'].data_ptr(), dev['bL'].data_ptr(), dev['v'].data_ptr(), attn.data_ptr(),
              hist.data_ptr(), B, Tx, S, ws.data_ptr(), ws.numel(), H._stream())
    assert torch.isfinite(hist).all() and torch.isfinite(attn).all()
    res = []
    for hs, at in ((hist64.float().contiguous().cuda(), attn64.float().contiguous().cuda()), (hist, attn)):
        args = (dev['ep'], dev['epq'], dev['P'], w_ih, dev['w_hh'], dev['b_hh'], dev['W'], dev['bW'], dev['cw'],
                dev['L'], dev['bL'], dev['v'], hs, at, dhist.cuda())
        outs = []
        for _ in range(2):
            bws = _poisoned_ws(_lib.query('ft_taco_attend_bwd_workspace', B, Tx, S))
            outs.append(H.taco_attend_bwd(*args, ws=bws, alloc=poison))
        torch.cuda.synchronize()
        for k in outs[0]:
            assert _same_bits(outs[0][k], outs[1][k]), ('not reproducible', k)
        res.append(outs[0])
    return res


ATT_CASES = [(B, Tx, S) for B in (1, 3, 17) for Tx in (1, 5, 31, 33, 70) for S in (1, 2, 7)]


@pytest.mark.parametrize('B,Tx,S', ATT_CASES, ids=['B%d-Tx%d-S%d' % c for c in ATT_CASES])
def test_attend_bwd_matches_float64_autograd(B, Tx, S):
    o, dhist = _att_operands(B, Tx, S)
    (r64, hist64, attn64), (r32, _, _) = _att_reference(o, dhist, torch.float64), _att_reference(o, dhist, torch.float32)
    got, chain = _att_gpu(o, dhist, hist64, attn64)
    _check('attend_bwd B %d Tx %d S %d' % (B, Tx, S), got, r64, r32)
    _check('  (device forward) B %d Tx %d S %d' % (B, Tx, S), chain, r64, r32, enforce=False)


def test_attend_bwd_long_sequence():
    """B = 3, Tx = 40, S = 60: the same bound; the error of dP per block of 10 steps shows growth with S.
    At randn * 0.7 the backward amplifies by ~1e36 over the 60 steps (|dP|inf per block of 10 steps, float64: 9e5, 3e10,
    2e18, 5e24, 1e30, 2e36) and the parameter sums pass 3.4e38: with a randn cotangent the stock float32 yardstick is
    inf / NaN and so is the bound.  The cotangent is therefore randn * 2^-100: a power of two, so every float64 figure
    is the randn figure times 2^-100 exactly and every float32 rounding is the one the randn run would make, only inside
    float32's range (elements below 2^-126 flush to zero, 1e-44 of the arrays' scale)."""
    B, Tx, S = 3, 40, 60
    o, dhist = _att_operands(B, Tx, S)
    dhist = dhist * 2.0 ** -100
    (r64, hist64, attn64), (r32, _, _) = _att_reference(o, dhist, torch.float64), _att_reference(o, dhist, torch.float32)
    assert all(bool(torch.isfinite(v).all()) for v in r32.values()), 'the float32 yardstick must be finite'
    got, chain = _att_gpu(o, dhist, hist64, attn64)
    dP = got['dP'].double().cpu()
    for s0 in range(0, S, 10):
        ref = r64['dP'][s0:s0 + 10]
        print('steps %2d..%2d  dP |x64|inf %.2e  stock fp32 %.2e  gpu %.2e'
              % (s0, s0 + 9, float(ref.abs().max()), float((r32['dP'][s0:s0 + 10].double() - ref).abs().max()),
                 float((dP[s0:s0 + 10] - ref).abs().max())))
    _check('attend_bwd long', got, r64, r32)
    _check('  (device forward) long', chain, r64, r32, enforce=False)


def test_attend_bwd_bad_arguments():
    assert _lib.query('ft_taco_attend_bwd_workspace', 2, 1025, 3) == 0
    assert _lib.query('ft_taco_attend_bwd_workspace', 2, 8, 0) == 0
    o, dhist = _att_operands(2, 8, 3)
    f = lambda *shape: torch.zeros(*shape, device='cuda')
    dev = {k: o[k].cuda() for k in ATT_KEYS}

    def call(Tx, S, ws_bytes):
        outs = [f(2, 8, D), f(2, 8, D), f(3, 2, 3 * D), f(3 * D, D), f(3 * D, D), f(3 * D), f(D, D), f(D), f(32, 2, 31),
                f(D, 32), f(D), f(D)]
        ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device='cuda')
        _lib.call('ft_taco_attend_bwd', *(dev[k].data_ptr() for k in ATT_KEYS[:4]), D,
                  *(dev[k].data_ptr() for k in ATT_KEYS[4:]), f(3, 2, 2 * D).data_ptr(), f(2, 3, 8).data_ptr(),
                  f(3, 2, 2 * D).data_ptr(), *(t.data_ptr() for t in outs), 2, Tx, S, ws.data_ptr(), ws_bytes,
                  H._stream())

    need = _lib.query('ft_taco_attend_bwd_workspace', 2, 8, 3)
    with pytest.raises(_lib.FtError, match='Tx must be in 1..1024'):
        call(1025, 3, need)
    with pytest.raises(_lib.FtError, match='S must be >= 1'):
        call(8, 0, need)
    with pytest.raises(_lib.FtError, match='workspace too small'):
        call(8, 3, need - 256)
    torch.cuda.synchronize()


# ---- zoneout LSTM ----------------------------------------------------------------------------------------------------
def _zone_mask(seed, S, B, L, p):
    """1.0 where the step is zoned (h keeps its previous value): where ft_dropout's mask of (p, seed) is 0"""
    keep = dropout_cpu.keep(seed, S * B * L, p).reshape(S, B, L)
    return torch.from_numpy((~keep).astype(np.float64))


def _zone_operands(L, B, S):
    g = torch.Generator().manual_seed(15485863 * L + 1031 * B + S)
    n = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32) * 0.7
    return dict(xp=n(S, B, 4 * L), w_hh=n(4 * L, L), b_hh=n(4 * L)), torch.randn(S, B, L, generator=g)


def _zone_reference(o, dout, m, dt):
    xp, w_hh, b_hh = (o[k].to(dt).requires_grad_(True) for k in ('xp', 'w_hh', 'b_hh'))
    S, B, G = xp.shape
    L = G // 4
    eye, zero = torch.eye(G, dtype=dt), torch.zeros(G, dtype=dt)
    h = c = xp.new_zeros(B, L)
    hs, cs = [], []
    for s in range(S):
        hc, c = K.lstm_cell(xp[s], h, c, eye, w_hh, zero, b_hh)
        ms = m[s].to(dt)
        h = ms * h + (1 - ms) * hc
        hs.append(h)
        cs.append(c)
    hs, cs = torch.stack(hs), torch.stack(cs)
    (hs * dout.to(dt)).sum().backward()
    return dict(h=hs.detach(), c=cs.detach(), dxp=xp.grad, dw_hh=w_hh.grad, db_hh=b_hh.grad)


def _zone_gpu(o, dout, p, seed):
    S, B, G = o['xp'].shape
    L = G // 4
    xp, w_hh, b_hh = (o[k].cuda() for k in ('xp', 'w_hh', 'b_hh'))
    outs = []
    for _ in range(2):
        gates, c, h = H.taco_lstm_zone_fwd(xp, w_hh, b_hh, p, seed, alloc=poison)
        ws = _poisoned_ws(_lib.query('ft_taco_lstm_zone_workspace', B, L))
        dxp = H.taco_lstm_zone_bwd(dout.cuda(), gates, c, H.transpose2d(w_hh), p, seed, ws=ws, alloc=poison)
        dw_hh = poison(G, L, device='cuda')
        H.linear_bwd_weight_raw(dxp.data_ptr(), G, h.data_ptr(), L, dw_hh, S * B, L, G, B=B, T=S, x_shift=-1,
                                dy_tm=True, x_tm=True)
        outs.append(dict(h=h, c=c, gates=gates, dxp=dxp, dw_hh=dw_hh, db_hh=H.colsum(dxp)))
    torch.cuda.synchronize()
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), ('not reproducible', k)
    return outs[0]


ZONE_CASES = [(L, B, S, p) for L in (40, 512) for B in (1, 3, 17) for S in (1, 2, 9) for p in (0.0, 0.1, 0.5)]


@pytest.mark.parametrize('L,B,S,p', ZONE_CASES, ids=['L%d-B%d-S%d-p%g' % c for c in ZONE_CASES])
def test_lstm_zone_matches_float64_autograd(L, B, S, p):
    seed = 0x1234567 * (L + 7 * B + 31 * S) * 0x9E3779B97F4A7C15 % 2 ** 62
    o, dout = _zone_operands(L, B, S)
    m = _zone_mask(seed, S, B, L, p)
    if p == 0.0:
        assert not bool(m.any())
    elif S * B * L >= 1000:
        assert 0.5 * p < float(m.mean()) < 1.5 * p, float(m.mean())
    r64, r32 = _zone_reference(o, dout, m, torch.float64), _zone_reference(o, dout, m, torch.float32)
    got = _zone_gpu(o, dout, p, seed)
    _check('lstm_zone L %d B %d S %d p %g' % (L, B, S, p), got, r64, r32)


def test_lstm_zone_all_zoned():
    """p = 1 zones every step: h stays 0, dW_hh is exactly 0, the cell state still runs"""
    L, B, S = 40, 3, 5
    o, dout = _zone_operands(L, B, S)
    m = _zone_mask(99 << 32, S, B, L, 1.0)
    assert bool(m.all())
    got = _zone_gpu(o, dout, 1.0, 99 << 32)
    assert not bool(got['h'].any()) and not bool(got['dw_hh'].any()) and not bool(got['dxp'].any())
    r64, r32 = _zone_reference(o, dout, m, torch.float64), _zone_reference(o, dout, m, torch.float32)
    assert float(r64['c'].abs().max()) > 0.1
    _check('lstm_zone all zoned', got, r64, r32)


def test_zoneout_lstm_fn_gradients():
    """taco_ops.ZoneoutLSTMFn (input projection + recurrence) under plain autograd: dx and the four parameter gradients"""
    L, B, S, p, seed = 40, 3, 9, 0.1, (77 << 32) + 5
    g = torch.Generator().manual_seed(5)
    n = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32) * 0.7
    o = dict(x=n(S, B, L), w_ih=n(4 * L, L), w_hh=n(4 * L, L), b_ih=n(4 * L), b_hh=n(4 * L))
    dout = torch.randn(S, B, L, generator=g)
    m = _zone_mask(seed, S, B, L, p)

    def ref(dt):
        t = {k: v.to(dt).requires_grad_(True) for k, v in o.items()}
        h = c = t['x'].new_zeros(B, L)
        hs = []
        for s in range(S):
            hc, c = K.lstm_cell(t['x'][s], h, c, t['w_ih'], t['w_hh'], t['b_ih'], t['b_hh'])
            h = m[s].to(dt) * h + (1 - m[s].to(dt)) * hc
            hs.append(h)
        hs = torch.stack(hs)
        (hs * dout.to(dt)).sum().backward()
        return dict(h=hs.detach(), **{'d' + k: v.grad for k, v in t.items()})

    t = {k: v.cuda().requires_grad_(True) for k, v in o.items()}
    h = taco_ops.ZoneoutLSTMFn.apply(t['x'], t['w_ih'], t['w_hh'], t['b_ih'], t['b_hh'], p, seed)
    (h * dout.cuda()).sum().backward()
    got = dict(h=h, **{'d' + k: v.grad for k, v in t.items()})
    _check('ZoneoutLSTMFn', got, ref(torch.float64), ref(torch.float32))


def test_lstm_zone_bad_arguments():
    f = lambda *shape: torch.zeros(*shape, device='cuda')
    with pytest.raises(_lib.FtError, match='multiple of 4'):
        _lib.call('ft_taco_lstm_zone_fwd', f(1, 1, 24).data_ptr(), f(24, 6).data_ptr(), f(24).data_ptr(), 0.1, 1,
                  f(1, 1, 24).data_ptr(), f(1, 1, 6).data_ptr(), f(1, 1, 6).data_ptr(), 1, 1, 6, H._stream())
    with pytest.raises(_lib.FtError, match='S must be >= 1'):
        _lib.call('ft_taco_lstm_zone_fwd', f(1, 1, 16).data_ptr(), f(16, 4).data_ptr(), f(16).data_ptr(), 0.1, 1,
                  f(1, 1, 16).data_ptr(), f(1, 1, 4).data_ptr(), f(1, 1, 4).data_ptr(), 1, 0, 4, H._stream())
    with pytest.raises(_lib.FtError, match='workspace too small'):
        _lib.call('ft_taco_lstm_zone_bwd', f(1, 1, 4).data_ptr(), f(1, 1, 16).data_ptr(), f(1, 1, 4).data_ptr(),
                  f(4, 16).data_ptr(), 0.1, 1, f(1, 1, 16).data_ptr(), 1, 1, 4, f(4).data_ptr(), 8, H._stream())
    torch.cuda.synchronize()
