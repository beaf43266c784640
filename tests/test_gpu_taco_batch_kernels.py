"""GPU: ft_taco_gen_batch_steps (csrc/ft_taco.hip: the attention kernels with lengths, the 16-item MFMA cells, the
per-item stop) through the C ABI, against tests/taco_step_cpu.py's gen_steps run PER ITEM in float64 on the item's own
slice ep[b, :n], epq[b, :n] -- the item alone.  Metric and bounds are those of tests/test_taco_step_cpu.py, imported
unchanged: per step, max |log attn - log ref| and max |x - ref|, against 8 x the carried error of the fp32 restatement
of the same item + 16 eps x max(1, |ref|) (+ 2e-7 sum|v| for log attn).  Every figure is printed (-s).

Shapes (B, Tx, lstm_dims, r, S): lstm_dims 512 (the template path) at B = 1 and 3; 40 (float4 loop) at exactly one
16-item tile; 37 (scalar loop) at B = 17, a second tile with one item; 258 with r = 20 (100 mel workgroups per tile
through the ticket counter).  Lengths: 1, one below / at / above the 32-token energy chunk, Tx itself, more than one
token chunk.

Every call runs twice: with NaN in every enc_proj / enc_pq row past an item's length, in w_ih's unread columns and in
the whole workspace (0xFF bytes), and with finite junk there instead; the valid outputs must be finite and must not
change by a bit, attn must be exactly 0 at t >= n.  A lengths-full B = 1 call agrees with ft_taco_gen_steps within the
same bounds."""
import pytest
import torch

import taco_step_cpu as K
from forwardtacotron_amd import _lib
from forwardtacotron_amd import hip as H
from test_gpu_taco_kernels import _Gen, _dev, _w_ih
from test_taco_step_cpu import bound, gen_operands, metric, run_gen

pytestmark = pytest.mark.gpu

D = 256
NAN = float('nan')
QUANT = ('attn', 'hist', 'P', 'frames')
# (B, Tx, lstm_dims, r, S) -> lengths
CASES = {
    (1, 33, 512, 1, 12): [33],
    (3, 33, 512, 2, 8): [1, 32, 33],
    (16, 40, 40, 3, 8): [40, 33, 32, 31, 17, 16, 15, 1, 2, 8, 40, 39, 24, 25, 9, 5],
    (17, 65, 37, 1, 8): [31, 64, 65, 1, 33, 32, 2, 48, 16, 15, 47, 65, 7, 63, 34, 20, 65],
    (2, 257, 258, 20, 3): [257, 130],
}


def _operands(case):
    """the operands of test_taco_step_cpu.gen_operands with ep, epq for B items"""
    B, Tx, Ld, r, S = case
    o = dict(gen_operands((Tx, Ld, r, S)))
    g = torch.Generator().manual_seed(1000 + 31 * B + Tx)
    o['ep'] = torch.randn(B, Tx, D, generator=g)
    o['epq'] = torch.randn(B, Tx, D, generator=g)
    return o


def _item(o, b, n):
    q = dict(o)
    q.update(ep=o['ep'][b:b + 1, :n], epq=o['epq'][b:b + 1, :n])
    return q


def _references(o, case, lens):
    """per item: (float64 result, bounds by quantity) of the item alone"""
    _, _, Ld, r, S = case
    out = []
    for b, n in enumerate(lens):
        q = _item(o, b, n)
        c1 = (n, Ld, r, S)
        r64, r32 = run_gen(q, c1, torch.float64), run_gen(q, c1, torch.float32)
        out.append((r64, {k: bound(k, r64, r32, o['v']) for k in QUANT}))
    return out


class _BatchGen:
    """device operands and poisoned outputs of one call of ft_taco_gen_batch_steps"""

    def __init__(self, o, case, lens, ld, threshold, poison):
        self.B, self.Tx, self.Ld, self.r, self.S = case
        B, Tx, S, r = self.B, self.Tx, self.S, self.r
        self.ld, self.thr = ld, threshold
        d = {k: _dev(v) for k, v in o.items() if k not in ('l1', 'l2', 'w_ih')}
        d['w_ih'] = _w_ih(o['w_ih'], D + 128, ld)
        d['l1'], d['l2'] = [_dev(t) for t in o['l1']], [_dev(t) for t in o['l2']]
        junk = torch.Generator().manual_seed(3)
        for k in ('ep', 'epq'):
            for b, n in enumerate(lens):
                d[k][b, n:] = NAN if poison else torch.randn(Tx - n, D, generator=junk).cuda()
        if not poison:
            d['w_ih'] = torch.nan_to_num(d['w_ih'], nan=0.5)
        self.d = d
        self.lens = torch.tensor(lens, dtype=torch.int64, device='cuda')
        self.out = dict(P=torch.full((S, B, 3 * D), NAN, device='cuda'), hist=torch.full((S, B, 2 * D), NAN, device='cuda'),
                        attn=torch.full((B, S, Tx), NAN, device='cuda'),
                        frames=torch.full((B, S * r, 80), NAN, device='cuda'))
        self.s_out = torch.full((B,), -1, dtype=torch.int32, device='cuda')
        nbytes = _lib.query('ft_taco_gen_batch_workspace', B, Tx, self.Ld, r)
        assert nbytes > 0
        self.ws = torch.full((nbytes,), 0xFF if poison else 0x3C, dtype=torch.uint8, device='cuda')

    def steps(self, s0, n):
        d, out = self.d, self.out
        p = lambda *ks: tuple(d[k].data_ptr() for k in ks)
        _lib.call('ft_taco_gen_batch_steps', *p('ep', 'epq', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'w_ih'), self.ld,
                  *p('b_ih', 'w_hh', 'b_hh', 'W', 'bW', 'cw', 'L', 'bL', 'v', 'rnn_in_w', 'rnn_in_b'),
                  *(t.data_ptr() for t in d['l1']), *(t.data_ptr() for t in d['l2']), d['mel_w'].data_ptr(),
                  float(self.thr), out['P'].data_ptr(), out['hist'].data_ptr(), out['attn'].data_ptr(),
                  out['frames'].data_ptr(), self.s_out.data_ptr(), self.lens.data_ptr(), self.B, self.Tx, self.Ld,
                  self.r, self.S, s0, n, self.ws.data_ptr(), self.ws.numel(), H._stream())
        return self

    def item(self, b, n):
        """item b's valid outputs in the layout of test_taco_step_cpu.run_gen"""
        o = self.out
        return dict(P=o['P'][:, b], hist=o['hist'][:, b], attn=o['attn'][b:b + 1, :, :n],
                    frames=o['frames'][b].reshape(self.S, -1))


@pytest.mark.parametrize('case', list(CASES), ids=['-'.join(map(str, c)) for c in CASES])
def test_batch_steps_match_every_item_alone_in_float64(case):
    B, Tx, Ld, r, S = case
    lens = CASES[case]
    assert len(lens) == B and max(lens) == Tx and min(lens) >= 1
    o = _operands(case)
    refs = _references(o, case, lens)
    run = _BatchGen(o, case, lens, 384, -1e9, True).steps(0, S // 2).steps(S // 2, S - S // 2)     # in two calls
    clean = _BatchGen(o, case, lens, 400, -1e9, False).steps(0, S)
    torch.cuda.synchronize()
    assert run.s_out.tolist() == [S] * B and clean.s_out.tolist() == [S] * B
    worst = {k: 0.0 for k in QUANT}
    bad = []
    for b, n in enumerate(lens):
        got, other = run.item(b, n), clean.item(b, n)
        r64, bounds = refs[b]
        assert not bool(run.out['attn'][b, :, n:].any()), b                  # exact zeros past the item's tokens
        for k in QUANT:
            assert bool(torch.isfinite(got[k]).all()), (b, k)
            assert torch.equal(got[k], other[k]), (b, k)                     # NaN or junk in what must not be read
            ratio = float((metric(k, got[k], r64[k]) / bounds[k]).max())
            worst[k] = max(worst[k], ratio)
            if ratio > 1.0:
                bad.append((b, n, k, ratio))
    print('batch B %d Tx %d lstm %d r %d S %d: worst step, gpu error / bound: %s'
          % (*case, ' '.join('%s %.2f' % (k, v) for k, v in worst.items())))
    assert not bad, bad


@pytest.mark.parametrize('case', list(CASES), ids=['-'.join(map(str, c)) for c in CASES])
def test_full_length_single_item_agrees_with_gen_steps(case):
    _, Tx, Ld, r, S = case
    o = _item(_operands(case), 0, Tx)
    c1 = (Tx, Ld, r, S)
    r64, r32 = run_gen(o, c1, torch.float64), run_gen(o, c1, torch.float32)
    bounds = {k: bound(k, r64, r32, o['v']) for k in QUANT}
    one, s_one = _Gen(o, c1, 384, -1e9).steps(0, S).result()
    run = _BatchGen(o, (1,) + c1, [Tx], 384, -1e9, True).steps(0, S)
    torch.cuda.synchronize()
    got = run.item(0, Tx)
    assert s_one == S and run.s_out.tolist() == [S]
    for k in QUANT:
        d_ref = float((metric(k, got[k], r64[k]) / bounds[k]).max())
        d_one = float((metric(k, got[k], one[k].double().cpu()) / bounds[k]).max())
        print('B = 1 full length Tx %d lstm %d r %d %-6s: vs float64 %.2f of the bound, vs ft_taco_gen_steps %.2f'
              % (Tx, Ld, r, k, d_ref, d_one))
        assert d_ref <= 1.0 and d_one <= 1.0, (k, d_ref, d_one)


def test_per_item_stop_records_each_items_first_step():
    """thresholds between two items' maxima: the item below stops at the first eligible step, the other never"""
    case = (3, 33, 512, 2, 8)
    lens = CASES[case]
    o = _operands(case)
    B, _, _, r, S = case
    full = _BatchGen(o, case, lens, 384, -1e9, True).steps(0, S)
    torch.cuda.synchronize()
    first = 10 // r + 1
    mx = full.out['frames'].reshape(B, S, -1).amax(2)[:, first]              # per item, at the first eligible step
    order = torch.argsort(mx).tolist()
    lo, hi = float(mx[order[0]]), float(mx[order[1]])
    assert hi - lo > 2e-3, (lo, hi)
    stop = _BatchGen(o, case, lens, 384, 0.5 * (lo + hi), True).steps(0, S)
    torch.cuda.synchronize()
    s_out = stop.s_out.tolist()
    assert s_out[order[0]] == first + 1 and all(s > first + 1 for i, s in enumerate(s_out) if i != order[0]), s_out
    for k in ('frames', 'attn', 'P', 'hist'):
        assert torch.equal(stop.out[k], full.out[k]), k                      # stopped items are stepped on
