"""CPU only: what tests/attn_cpu.py claims, proven on the inputs of tests/test_gpu_attn_train.py.

  * reference() is torch's float64 autograd of masked softmax attention with the given dropout mask;
  * emulate() in fp32 with the key / query blocks summed in reverse order -- a legitimate other summation order -- stays
    inside the bar the GPU tests give the kernels, 4 E + 16 * 2^-24 * max(1, max|ref|) per (item, head) slab;
  * every wrong variant emulate() can switch on leaves that bar, on an output it can affect, in every case where it
    changes anything at all.  "Leaves the bar" is `not (error <= bar)`, the negation of what the GPU tests assert: a NaN
    slab (the only valid key of an item lost) counts.

Sites: 'fwd', 'dq', 'dkv' are the three kernels; the mask index and the key mask are written out separately in each, so
those variants are switched on in one kernel at a time and have to show in that kernel's own outputs (a wrong forward
also moves the gradients through att and lse2; it is held to att / lse2 alone here)."""
import math

import pytest
import torch

import attn_cpu as A

_cache = {}


def _case(name):
    """inputs, reference, emulation and the bars of one case, computed once"""
    if name not in _cache:
        c = A.make_case(name)
        ref = A.reference(*A.args(c))
        emu = A.emulate(*A.args(c))
        bars = {o: A.slab_bar(o, emu[o], ref[o], c['nh'])[0] for o in A.OUTPUTS}
        _cache[name] = (c, ref, emu, bars)
    return _cache[name]


def _autograd(c):
    qkv, datt, key_pad, nh, scale, keep = A.args(c)
    B, T, d3 = qkv.shape
    d = d3 // 3
    hd = d // nh
    q, k, v = [t.bfloat16().double().reshape(B, T, nh, hd).permute(0, 2, 1, 3).clone().requires_grad_(True)
               for t in qkv.split(d, dim=-1)]
    s = (q @ k.transpose(-1, -2)) * scale
    if key_pad is not None:
        s = s.masked_fill(key_pad.bool()[:, None, None, :], float('-inf'))
    P = torch.softmax(s, dim=-1) * torch.as_tensor(keep)
    o = (P @ v).permute(0, 2, 1, 3).reshape(B, T, d)
    (o * datt.double()).sum().backward()
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B, T, d)
    return dict(att=o.detach(), lse2=torch.logsumexp(s.detach(), dim=-1) / math.log(2.0), dq=rows(q.grad), dk=rows(k.grad),
                dv=rows(v.grad))


@pytest.mark.parametrize('name', list(A.CASES))
def test_reference_equals_float64_autograd(name):
    c, ref, _, _ = _case(name)
    want = _autograd(c)
    for o in A.OUTPUTS:
        err, top = float((ref[o] - want[o]).abs().max()), float(want[o].abs().max())
        assert err <= 1e-12 * top, (o, err, top)


def test_single_key_gradients_are_exactly_zero_in_float64():
    """L = 1: P = 1, dS = dP - dP.  What the kernels leave there is rounding alone (delta from the fp32 datt, dP from
    the bf16 one), and emulate() reproduces it: O(2^-9 |dO| |v|), not 0."""
    for name in ('edges-hd64-p0.0', 'edges-hd128-p0.1'):
        c, ref, emu, _ = _case(name)
        assert A.EDGE_LENS[0] == 1
        for o in ('dq', 'dk'):
            assert float(ref[o][0].abs().max()) == 0.0
            res = float(emu[o][0].abs().max())
            d = c['nh'] * c['hd']
            q, k, v = (float(t.abs().max()) for t in c['qkv'][0].split(d, dim=-1))
            # |dS| <= scale * hd terms * 2^-8 (datt to bf16, then dS to bf16) * |dO| |v|; dq = dS k, dk = sum_q dS q
            ds = c['scale'] * c['hd'] * 2.0 ** -8 * float(c['datt'][0].abs().max()) * v
            bound = ds * k if o == 'dq' else ds * c['T'] * q
            print(f'{name} {o}: emulated residue {res:.2e}, bound from the formats {bound:.2e}')
            assert 0 < res <= bound


@pytest.mark.parametrize('name', list(A.CASES))
def test_fp32_in_reverse_block_order_stays_inside_the_bar(name):
    c, ref, _, bars = _case(name)
    alt = A.emulate(*A.args(c), acc=torch.float32, reverse=True)
    for o in A.OUTPUTS:
        ratio = float((A.slab_err(o, alt[o], ref[o], c['nh']) / bars[o]).max())
        print(f'{name} {o}: fp32 / reversed blocks at {ratio:.2f} of the bar')
        assert ratio <= 1.0, (o, ratio)


# (mutation, sites switched on together, outputs it has to show in)
_MASKED = [(m, (s,), outs) for m in ('last_key', 'key64', 'mask_shift', 'mask_swap', 'mask_nohead')
           for s, outs in (('fwd', ('att', 'lse2')), ('dq', ('dq',)), ('dkv', ('dk', 'dv')))]
PLAN = _MASKED + [
    ('no_delta', A.SITES, ('dq', 'dk')),
    ('delta_all_heads', A.SITES, ('dq', 'dk')),
    ('keep_on_p', ('dq',), ('dq',)), ('keep_on_p', ('dkv',), ('dk',)),
    ('no_scale', ('dq',), ('dq',)), ('no_scale', ('dkv',), ('dk',)),
    ('lse_natural', ('fwd',), ('lse2',)),
    ('l_after_dropout', ('fwd',), ('att',)),
]


def _not_applicable(mut, where, c):
    """the reason a mutation changes nothing in case c, or None"""
    if c['p'] == 0 and (mut.startswith('mask_') or mut in ('keep_on_p', 'l_after_dropout')):
        return 'p = 0: no mask is drawn'
    if c['nh'] == 1 and mut in ('mask_nohead', 'delta_all_heads'):
        return 'one head: inst == b'
    if mut == 'key64' and (c['T'] <= A.KB or (c['key_pad'] is not None and bool(c['key_pad'][:, A.KB].all()))):
        return 'no item has a valid key 64'
    if mut == 'mask_swap' and c['T'] == 1:
        return 'T = 1: q == k'
    if mut == 'last_key' and where == ('dq',) and c['T'] == 1:
        return 'T = 1: the exact dq is 0, and so is the dq of a kernel that lost its only key'
    return None


@pytest.mark.parametrize('mut,where,outs', PLAN, ids=[f'{m}-{"+".join(w)}' for m, w, _ in PLAN])
def test_every_mutation_leaves_the_bar(mut, where, outs):
    smallest, skipped = float('inf'), {}
    for name in A.CASES:
        c, ref, _, bars = _case(name)
        why = _not_applicable(mut, where, c)
        if why:
            skipped.setdefault(why, []).append(name)
            continue
        bad = A.emulate(*A.args(c), mutate=mut, where=where)
        best = 0.0
        for o in outs:
            ratio = A.slab_err(o, bad[o], ref[o], c['nh']) / bars[o]
            ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio)
            best = max(best, float(ratio.max()))
        assert best > 1.0, (name, best)
        smallest = min(smallest, best)
    print(f'{mut} in {"+".join(where)}: worst slab at >= {smallest:.1f} x the bar in every applicable case')
    for why, names in skipped.items():
        print(f'  not applicable ({why}): {len(names)} cases')
    assert smallest > 1.0
