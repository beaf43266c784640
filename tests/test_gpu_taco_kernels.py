"""GPU: the kernels of csrc/ft_taco.hip, called through the C ABI, against tests/taco_step_cpu.py in float64.

ft_taco_attend (GRU cell + query slabs, LSA energies, softmax + context) and ft_taco_gen_steps (those three between the
prenet, rnn_input, the two LSTM cells and mel_proj with the stop test) are compared step by step in the metric and under
the bounds that tests/test_taco_step_cpu.py builds and proves sound: max |log attn - log ref| and max |x - ref| per
step, against 8 x the error of the fp32 restatement on the host + 16 epsilons x max(1, |ref|) (+ 2e-7 sum|v| for
log attn, the kernel header's bound of its hardware tanh).  Nothing is hard-coded; every figure is printed (-s).

Shapes.  ft_taco_attend, S = 8: Tx = 1; 15 / 16 (the 31-wide window over both paddings); 31 / 32 / 33 (the 32-token
energy chunk); 192 / 193 (the context kernel's prefetched enc_pq rows), 217 / 224 / 225 (its 4-way unrolled tail: first
token group, every group, one past), 256 / 257 (one and two softmax tokens per thread), 1024 (the bound); B = 1, 15, 16,
17, 33 (batch tiles of 16, a partly full second and third one).  ft_taco_gen_steps: lstm_dims 512 (templated dot
products), 300 (float4 loop, two iterations), 37 and 258 (scalar loop, one and two iterations), r = 20 (400 mel
workgroups through the ticket counter), Tx = 1024.

Every call gets w_ih with NaN in the columns it must not read (256.. for attend, 384.. for generate, ld_w_ih 384 and
400), a workspace of 0xFF bytes and NaN outputs: finite outputs prove that it reads nothing it did not write.  The ring
(no history) must give the history run's attention bit for bit; two calls over [0, 5) and [5, 12) the single call's
outputs; a stop at s* the never-stop run's slots <= s*.  ft_taco_frames and ft_taco_add: equality with indexing and
addition, past the grid-stride threshold of 256 * 1024 elements.

Measured on an MI355X (largest per-step error over a case's steps, range over the cases):
                    fp32 restatement      kernels               kernels / bound, worst step
  attend  log attn  1.8e-6 .. 4.5e-6      1.3e-6 .. 3.8e-6      <= 0.05        (Tx = 1: 0 and 0)
          hist      5.3e-7 .. 2.8e-6      3.1e-7 .. 2.0e-6      <= 0.14
  generate log attn 1.3e-6 .. 4.1e-6      5.2e-7 .. 2.8e-6      <= 0.05
          hist      4.7e-7 .. 1.7e-6      2.6e-7 .. 1.2e-6      <= 0.14
          P         2.1e-7 .. 8.0e-7      1.4e-7 .. 4.1e-7      <= 0.09
          frames    4.9e-7 .. 1.7e-6      2.4e-7 .. 9.7e-7      <= 0.14
No case needs more than the fp32 restatement's own error.  Four numerically wrong builds of the kernels were each caught
where expected: a dropped term of the context kernel's unrolled tail by every case with Tx >= 217 and by no other; the
last token missing from the location window by every attend case with Tx > 1 and five of six generate cases; a dropped
query slab by every case with Tx > 1; a dropped last element of the scalar dot-product loop by lstm_dims 37 and 258
only."""
import math

import pytest
import torch

from forwardtacotron_amd import _lib
from forwardtacotron_amd import hip as H
from test_taco_step_cpu import (ATTEND_CASES, GEN_CASES, S_ATT, STOP_CASE, attend_reference, gen_reference, metric,
                                stop_step)

pytestmark = pytest.mark.gpu

D = 256
NAN = float('nan')


def _dev(t):
    return t.contiguous().cuda()


def _w_ih(w, used, ld):
    """[768, ld] with NaN past the `used` columns the call may read"""
    out = torch.full((w.shape[0], ld), NAN, device='cuda')
    out[:, :used] = w[:, :used].cuda()
    return out


def _poisoned_ws(nbytes):
    assert nbytes > 0
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device='cuda')


def _report(what, got, r64, r32, bounds):
    """print and assert the per-step errors of every quantity in `bounds`"""
    bad = []
    for k, b in bounds.items():
        assert torch.isfinite(got[k]).all(), (what, k)
        err, e32 = metric(k, got[k], r64[k]), metric(k, r32[k], r64[k])
        print('%s %-6s fp32 restatement %.2e  gpu %.2e  bound %.2e  (worst step: gpu / bound %.2f)'
              % (what, 'log attn' if k == 'attn' else k, float(e32.max()), float(err.max()), float(b.max()),
                 float((err / b).max())))
        if bool((err > b).any()):
            bad.append((k, err.tolist(), b.tolist()))
    assert not bad, (what, bad)


# ---- ft_taco_attend -------------------------------------------------------------------------------------------------
def _attend(o, ld, keep_history):
    B, Tx = o['ep'].shape[:2]
    S = o['P'].shape[0]
    dev = {k: _dev(o[k]) for k in ('ep', 'epq', 'P', 'w_hh', 'b_hh', 'W', 'bW', 'cw', 'L', 'bL', 'v')}
    w_ih = _w_ih(o['w_ih'], D, ld)
    attn = torch.full((B, S, Tx), NAN, device='cuda')
    hist = torch.full((S, B, 2 * D), NAN, device='cuda') if keep_history else None
    ws = _poisoned_ws(_lib.query('ft_taco_attend_workspace', B, Tx))
    _lib.call('ft_taco_attend', dev['ep'].data_ptr(), dev['epq'].data_ptr(), dev['P'].data_ptr(), w_ih.data_ptr(), ld,
              dev['w_hh'].data_ptr(), dev['b_hh'].data_ptr(), dev['W'].data_ptr(), dev['bW'].data_ptr(),
              dev['cw'].data_ptr(), dev['L'].data_ptr(), dev['bL'].data_ptr(), dev['v'].data_ptr(), attn.data_ptr(),
              H._p(hist), B, Tx, S, ws.data_ptr(), ws.numel(), H._stream())
    torch.cuda.synchronize()
    return dict(attn=attn, hist=hist)


ATTEND_RUNS = [(c, 384) for c in ATTEND_CASES] + [((17, 257), 400)]
RING_CASES = [(17, 257), (2, 225)]


@pytest.mark.parametrize('case,ld', ATTEND_RUNS, ids=['%d-%d-ld%d' % (*c, ld) for c, ld in ATTEND_RUNS])
def test_attend_matches_float64(case, ld):
    o, r64, r32, bounds = attend_reference(case)
    got = _attend(o, ld, True)
    assert got['attn'].shape == r64['attn'].shape and got['hist'].shape == (S_ATT, case[0], 2 * D)
    _report('attend B %d Tx %d ld %d' % (*case, ld), got, r64, r32, bounds)
    if case in RING_CASES:
        ring = _attend(o, ld, False)
        assert torch.equal(ring['attn'], got['attn'])


# ---- ft_taco_gen_steps -----------------------------------------------------------------------------------------------
class _Gen:
    """device operands and poisoned outputs of one generate case; steps(s0, n) enqueues ft_taco_gen_steps"""

    def __init__(self, o, case, ld, threshold):
        self.Tx, self.Ld, self.r, self.S = case
        self.ld, self.thr = ld, threshold
        d = {k: _dev(v) for k, v in o.items() if k not in ('l1', 'l2', 'w_ih')}
        d['w_ih'] = _w_ih(o['w_ih'], D + 128, ld)
        d['l1'], d['l2'] = [_dev(t) for t in o['l1']], [_dev(t) for t in o['l2']]
        self.d = d
        S, r = self.S, self.r
        self.out = dict(P=torch.full((S, 3 * D), NAN, device='cuda'), hist=torch.full((S, 2 * D), NAN, device='cuda'),
                        attn=torch.full((1, S, self.Tx), NAN, device='cuda'),
                        frames=torch.full((S * r, 80), NAN, device='cuda'))
        self.s_out = torch.full((1,), -1, dtype=torch.int32, device='cuda')
        self.ws = _poisoned_ws(_lib.query('ft_taco_gen_workspace', self.Tx, self.Ld, r))

    def steps(self, s0, n):
        d, out = self.d, self.out
        p = lambda *ks: tuple(d[k].data_ptr() for k in ks)
        _lib.call('ft_taco_gen_steps', *p('ep', 'epq', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'w_ih'), self.ld,
                  *p('b_ih', 'w_hh', 'b_hh', 'W', 'bW', 'cw', 'L', 'bL', 'v', 'rnn_in_w', 'rnn_in_b'),
                  *(t.data_ptr() for t in d['l1']), *(t.data_ptr() for t in d['l2']), d['mel_w'].data_ptr(),
                  float(self.thr), out['P'].data_ptr(), out['hist'].data_ptr(), out['attn'].data_ptr(),
                  out['frames'].data_ptr(), self.s_out.data_ptr(), self.Tx, self.Ld, self.r, self.S, s0, n,
                  self.ws.data_ptr(), self.ws.numel(), H._stream())
        return self

    def result(self):
        torch.cuda.synchronize()
        got = dict(self.out)
        got['frames'] = got['frames'].reshape(self.S, -1)
        return got, int(self.s_out.item())


GEN_RUNS = [(c, 384) for c in GEN_CASES] + [(GEN_CASES[0], 400)]


@pytest.mark.parametrize('case,ld', GEN_RUNS, ids=['%d-%d-%d-%d-ld%d' % (*c, ld) for c, ld in GEN_RUNS])
def test_gen_steps_match_float64(case, ld):
    o, r64, r32, bounds = gen_reference(case)
    S = case[3]
    got, s_out = _Gen(o, case, ld, -1e9).steps(0, S).result()
    assert s_out == S
    _report('generate Tx %d lstm %d r %d S %d ld %d' % (*case, ld), got, r64, r32, bounds)


def test_gen_steps_in_two_calls_equal_one_call():
    o = gen_reference(STOP_CASE)[0]
    S = STOP_CASE[3]
    one, s_one = _Gen(o, STOP_CASE, 384, -1e9).steps(0, S).result()
    two, s_two = _Gen(o, STOP_CASE, 384, -1e9).steps(0, 5).steps(5, S - 5).result()
    assert s_one == s_two == S
    for k in one:
        assert torch.isfinite(two[k]).all() and torch.equal(one[k], two[k]), k


def test_gen_steps_stop():
    o, r64, _, _ = gen_reference(STOP_CASE)
    _, _, r, S = STOP_CASE
    s_star, thr = stop_step(r64['smax'], r)
    full, s_full = _Gen(o, STOP_CASE, 384, -1e9).steps(0, S).result()
    stop, s_stop = _Gen(o, STOP_CASE, 384, thr).steps(0, S).result()
    gpu_max = full['frames'].amax(1).tolist()
    print('stop: s* %d, threshold %.6f, float64 maxima %s, gpu maxima %s'
          % (s_star, thr, ['%.4f' % v for v in r64['smax'].tolist()], ['%.4f' % v for v in gpu_max]))
    assert s_full == S and s_stop == s_star + 1
    n = s_star + 1
    assert torch.equal(stop['frames'][:n], full['frames'][:n]) and torch.equal(stop['attn'][:, :n], full['attn'][:, :n])


# ---- ft_taco_frames, ft_taco_add -------------------------------------------------------------------------------------
def _frames(mel, r, S, n_mels):
    B, _, Tm = mel.shape
    out = torch.full((S, B, n_mels), NAN, device='cuda')
    _lib.call('ft_taco_frames', mel.data_ptr(), B, n_mels, Tm, r, S, out.data_ptr(), H._stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('B,n_mels,Tm,r', [(3, 80, 7, 1), (2, 80, 10, 3), (5, 7, 11, 3), (2, 80, 41, 20),
                                           (64, 80, 60, 1)])
def test_frames_equal_indexing(B, n_mels, Tm, r):
    mel = torch.randn(B, n_mels, Tm, generator=torch.Generator().manual_seed(Tm)).cuda()

    def want(S):
        w = torch.zeros(S, B, n_mels, device='cuda')
        w[1:] = mel[:, :, torch.arange(1, S, device='cuda') * r - 1].permute(2, 0, 1)
        return w

    S = math.ceil(Tm / r)
    if B == 64:
        assert S * B * n_mels > 256 * 1024          # the grid-stride loop
    out = _frames(mel, r, S, n_mels)
    assert torch.equal(out, want(S)) and not out[0].any()
    # the entry admits every step whose frame (S - 1) r - 1 exists and refuses the first that does not
    S_bad = math.ceil((Tm + 1) / r) + 1
    assert (S_bad - 1) * r - 1 >= Tm > (S_bad - 2) * r - 1
    assert torch.equal(_frames(mel, r, S_bad - 1, n_mels), want(S_bad - 1))
    with pytest.raises(_lib.FtError, match='taco_frames'):
        _frames(mel, r, S_bad, n_mels)


@pytest.mark.parametrize('n', [0, 1, 256 * 1024 + 37])
def test_add_equals_addition(n):
    g = torch.Generator().manual_seed(n)
    x, y = torch.randn(n + 3, generator=g).cuda(), torch.randn(n + 3, generator=g).cuda()
    out = torch.full((n + 3,), NAN, device='cuda')
    _lib.call('ft_taco_add', x.data_ptr(), y.data_ptr(), out.data_ptr(), n, H._stream())
    torch.cuda.synchronize()
    assert torch.equal(out[:n], x[:n] + y[:n]) and bool(torch.isnan(out[n:]).all())
