"""CPU: the inputs, the metric and the bounds of tests/test_gpu_taco_kernels.py are sound (no GPU).

That module holds the kernels of csrc/ft_taco.hip to tests/taco_step_cpu.py in float64, step by step, in
    log attn    max |log a - log ref| over items and tokens: a shift d of one token's energy shows as ~d whatever mass
                the token has, where plain attn shows it scaled by that mass
    hist, P, frames   max |a - ref|
with a bound that is measured, not chosen: the same restatement in fp32 (torch on the host) against float64, in the same
metric, step by step.  bound[s] = 8 x the largest fp32 error of the steps <= s (a recurrence carries its error forward,
so the error of a step is not bounded by one sample of the same step alone) + 16 fp32 epsilons x max(1, largest |ref|
of the step) (a case whose fp32 restatement is exact, Tx = 1, must not demand bit equality) and, for log attn alone,
+ 2e-7 sum|v|, the bound csrc/ft_taco.hip states for its hardware tanh.

This module builds the operands (seeded, the scales below), the float64 and fp32 references (once per case and process,
shared with the GPU module) and the bounds, and asserts for every case that
  * every float64 attention value is >= 1e-12, so the logarithm of the fp32 value is that of a normal number;
  * the metric sees every operand class of the LSA: one element of the location conv at its outermost taps (0 and 30; at
    Tx < 16 those two only ever meet the zero padding, changing them must change NOTHING, and the outermost taps that do
    meet a token, 16 - Tx and 14 + Tx, stand in), both channels, column 255 of W, L[255, 31] and v[255], each changed by
    0.05 (the column zeroed), move log attn at some step by >= 10 x that step's bound.  At Tx = 1 the softmax is the
    constant 1 and no LSA operand can move anything: asserted as such;
  * an item sliced out of a batch equals the item run alone to 1e-12 (float64): no arithmetic crosses items.

Scales: ep, epq, P ~ N(0,1); w_ih, w_hh, W ~ N(0,1)/16; biases 0.3 N; cw 0.3 N; L, v 0.25 N: the attention rows
have maxima of 0.07..0.9, and the location conv and `cumulative` carry real weight in the energies.  Generate cases:
N(0,1)/sqrt(fan_in) for the prenet, rnn_input, the LSTM weights and mel_proj, 0.3 N for their biases."""
import functools

import pytest
import torch

import taco_step_cpu as K

D = 256
S_ATT = 8
# ft_taco_attend: (B, Tx)
ATTEND_CASES = [(2, 1), (3, 15), (3, 16), (3, 31), (3, 32), (17, 33), (1, 40), (15, 40), (16, 40), (33, 31), (2, 192),
                (2, 193), (2, 217), (2, 224), (2, 225), (2, 256), (17, 257), (1, 1024)]
# ft_taco_gen_steps: (Tx, lstm_dims, r, S)
GEN_CASES = [(33, 512, 1, 12), (225, 300, 2, 8), (40, 37, 3, 12), (257, 258, 1, 8), (9, 40, 20, 3), (1024, 512, 1, 4)]
STOP_CASE = (40, 37, 3, 12)
# a case whose default seed misses a condition on the INPUTS (asserted below) names another one here
SEEDS = {(9, 40, 20, 3): 6}      # 3 steps: tokens 0 and 8 need attention mass by step 1 for the edge taps to count
EPS = float(torch.finfo(torch.float32).eps)
ATT_KEYS = ('ep', 'epq', 'P', 'w_ih', 'w_hh', 'b_hh', 'W', 'bW', 'cw', 'L', 'bL', 'v')


def _seed(case):
    return SEEDS.get(case, 7 + sum(int(c) * m for c, m in zip(case, (1, 1031, 1000003, 15485863))))


def _lsa_operands(g, B, Tx):
    n = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)
    return dict(ep=n(B, Tx, D), epq=n(B, Tx, D), w_hh=n(3 * D, D) / 16, b_hh=0.3 * n(3 * D), W=n(D, D) / 16,
                bW=0.3 * n(D), cw=0.3 * n(32, 2, 31), L=0.25 * n(D, 32), bL=0.3 * n(D), v=0.25 * n(D))


def attend_operands(case):
    """fp32 operands of taco_step_cpu.attend by name; w_ih is [768, 256], the columns the attention reads"""
    B, Tx = case
    g = torch.Generator().manual_seed(_seed(case))
    o = _lsa_operands(g, B, Tx)
    o['P'] = torch.randn(S_ATT, B, 3 * D, generator=g, dtype=torch.float32)
    o['w_ih'] = torch.randn(3 * D, D, generator=g, dtype=torch.float32) / 16
    return o


def gen_operands(case):
    """fp32 operands of taco_step_cpu.gen_steps by name; w_ih is [768, 384]"""
    Tx, Ld, r, S = case
    g = torch.Generator().manual_seed(_seed(case))
    n = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)
    o = _lsa_operands(g, 1, Tx)
    o.update(w_ih=n(3 * D, D + 128) / 16, b_ih=0.3 * n(3 * D),
             fc1_w=n(256, 80) / 80 ** 0.5, fc1_b=0.3 * n(256), fc2_w=n(128, 256) / 16, fc2_b=0.3 * n(128),
             rnn_in_w=n(Ld, 2 * D) / (2 * D) ** 0.5, rnn_in_b=0.3 * n(Ld), mel_w=n(80 * K.MAX_R, Ld) / Ld ** 0.5)
    for k in ('l1', 'l2'):
        o[k] = (n(4 * Ld, Ld) / Ld ** 0.5, n(4 * Ld, Ld) / Ld ** 0.5, 0.3 * n(4 * Ld), 0.3 * n(4 * Ld))
    return o


def _cast(x, dt):
    return tuple(t.to(dt) for t in x) if isinstance(x, tuple) else x.to(dt)


def run_attend(o, dt):
    """-> dict(attn [B,S,Tx], hist [S,B,512])"""
    attn, hist = K.attend(*(_cast(o[k], dt) for k in ATT_KEYS))
    return dict(attn=attn, hist=hist)


GEN_KEYS = ('ep', 'epq', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'w_ih', 'b_ih', 'w_hh', 'b_hh', 'W', 'bW', 'cw', 'L', 'bL',
            'v', 'rnn_in_w', 'rnn_in_b', 'l1', 'l2', 'mel_w')


def run_gen(o, case, dt):
    """-> dict(P [S,768], hist [S,512], attn [1,S,Tx], frames [S,r*80] (step-major), smax [S])"""
    _, _, r, S = case
    P, hist, attn, frames, smax = K.gen_steps(*(_cast(o[k], dt) for k in GEN_KEYS), r, S)
    return dict(P=P, hist=hist, attn=attn[None], frames=frames.reshape(S, -1), smax=smax)


# ---- metric and bounds ----------------------------------------------------------------------------------------------
def step_max(x, step_dim=0):
    """[.., S, ..] -> [S]: the largest entry of every step"""
    return x.movedim(step_dim, 0).reshape(x.shape[step_dim], -1).amax(1)


def metric(name, a, ref):
    """per-step error [S] of quantity `name` (float64 arithmetic on whatever precision a and ref hold)"""
    a, ref = a.double().cpu(), ref.double()
    if name == 'attn':
        return step_max((a.log() - ref.log()).abs(), 1)
    return step_max((a - ref).abs())


def scale(name, ref):
    return step_max(ref.log().abs(), 1) if name == 'attn' else step_max(ref.abs())


def bound(name, r64, r32, v):
    """per-step bound [S] (module docstring)"""
    carried = torch.cummax(metric(name, r32[name], r64[name]), 0).values
    b = 8 * carried + 16 * EPS * scale(name, r64[name]).clamp(min=1.0)
    return b + 2e-7 * float(v.double().abs().sum()) if name == 'attn' else b


@functools.lru_cache(maxsize=None)
def attend_reference(case):
    """(operands, float64 result, fp32 result, bounds by quantity): computed once, never modified"""
    o = attend_operands(case)
    r64, r32 = run_attend(o, torch.float64), run_attend(o, torch.float32)
    return o, r64, r32, {k: bound(k, r64, r32, o['v']) for k in ('attn', 'hist')}


@functools.lru_cache(maxsize=None)
def gen_reference(case):
    o = gen_operands(case)
    r64, r32 = run_gen(o, case, torch.float64), run_gen(o, case, torch.float32)
    return o, r64, r32, {k: bound(k, r64, r32, o['v']) for k in ('attn', 'hist', 'P', 'frames')}


def stop_step(smax, r):
    """(s*, threshold) of the stop test: the first step s* with s* r > 10, s* < S - 1 and an earlier step with s r > 10,
    whose maximum undercuts the running minimum over those earlier steps by >= 2e-3; the threshold lies midway, so
    >= 1e-3 from either.  None when the case has no such step."""
    S = smax.numel()
    first = 10 // r + 1
    for s in range(first + 1, S - 1):
        before = float(smax[first:s].min())
        if float(smax[s]) <= before - 2e-3:
            return s, 0.5 * (float(smax[s]) + before)
    return None


# ---- the assertions --------------------------------------------------------------------------------------------------
def _ids(cases):
    return ['-'.join(map(str, c)) for c in cases]


def _perturbations(o, Tx):
    """name -> (operands, must move): one operand element changed"""
    def with_(key, f):
        q = dict(o)
        q[key] = o[key].clone()
        f(q[key])
        return q

    def add(key, idx):
        def f(t):
            t[idx] += 0.05
        return with_(key, f)

    def zero_col(t):
        t[:, 255] = 0

    out = {}
    lo, hi = max(0, 16 - Tx), min(30, 14 + Tx)          # the outermost taps that meet a token
    for ch, filt in ((0, 0), (1, 31)):
        for tap in (0, 30, lo, hi):
            out[f'cw[{filt},{ch},{tap}]'] = (add('cw', (filt, ch, tap)), Tx > 1 and lo <= tap <= hi)
    out['W[:,255]=0'] = (with_('W', zero_col), Tx > 1)
    out['L[255,31]'] = (add('L', (255, 31)), Tx > 1)
    out['v[255]'] = (add('v', (255,)), Tx > 1)
    return out


def _check_inputs_and_metric(o, r64, bounds, rerun, Tx):
    attn = r64['attn']
    assert float(attn.min()) >= 1e-12, float(attn.min())
    assert torch.isfinite(bounds['attn']).all() and float(bounds['attn'].max()) < 1e-3, bounds['attn']
    for name, (q, must_move) in _perturbations(o, Tx).items():
        moved = metric('attn', rerun(q)['attn'], attn)
        if must_move:
            ratio = float((moved / bounds['attn']).max())
            assert ratio >= 10.0, (name, ratio, moved, bounds['attn'])
        else:
            assert float(moved.max()) == 0.0, (name, moved)


@pytest.mark.parametrize('case', ATTEND_CASES, ids=_ids(ATTEND_CASES))
def test_attend_case_inputs_metric_and_item_independence(case):
    B, Tx = case
    o, r64, r32, bounds = attend_reference(case)
    print(case, 'attn min %.2e, row maxima %.2f..%.2f' % (float(r64['attn'].min()), float(r64['attn'].amax(2).min()),
                                                           float(r64['attn'].amax(2).max())),
          'fp32 error: log attn %.2e, hist %.2e' % (float(metric('attn', r32['attn'], r64['attn']).max()),
                                                   float(metric('hist', r32['hist'], r64['hist']).max())),
          'bound: log attn %.2e, hist %.2e' % (float(bounds['attn'].max()), float(bounds['hist'].max())))
    _check_inputs_and_metric(o, r64, bounds, lambda q: run_attend(q, torch.float64), Tx)
    for b in sorted({0, min(16, B - 1), B - 1}):
        q = dict(o)
        q.update(ep=o['ep'][b:b + 1], epq=o['epq'][b:b + 1], P=o['P'][:, b:b + 1])
        alone = run_attend(q, torch.float64)
        assert float((alone['attn'][0] - r64['attn'][b]).abs().max()) <= 1e-12, b
        assert float((alone['hist'][:, 0] - r64['hist'][:, b]).abs().max()) <= 1e-12, b


@pytest.mark.parametrize('case', GEN_CASES, ids=_ids(GEN_CASES))
def test_generate_case_inputs_and_metric(case):
    Tx = case[0]
    o, r64, r32, bounds = gen_reference(case)
    print(case, 'attn min %.2e' % float(r64['attn'].min()),
          ' '.join('%s: fp32 error %.2e, bound %.2e' % (k, float(metric(k, r32[k], r64[k]).max()), float(b.max()))
                   for k, b in bounds.items()))
    _check_inputs_and_metric(o, r64, bounds, lambda q: run_gen(q, case, torch.float64), Tx)


def test_stop_case_has_a_stop_step():
    """the GPU stop test needs a step whose maximum is a new minimum among the eligible steps by a margin that the
    kernels' error (the frames bound, asserted here to be 10 x smaller) cannot close"""
    _, r64, _, bounds = gen_reference(STOP_CASE)
    _, _, r, S = STOP_CASE
    found = stop_step(r64['smax'], r)
    assert found is not None, r64['smax']
    s, thr = found
    assert s * r > 10 and s < S - 1
    assert float(bounds['frames'].max()) <= 1e-4
    assert all(float(r64['smax'][i]) >= thr + 1e-3 for i in range(10 // r + 1, s))
    assert float(r64['smax'][s]) <= thr - 1e-3
