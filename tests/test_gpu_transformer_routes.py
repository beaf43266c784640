"""FastPitch's bf16 transformer routes, gradient by gradient.

In bf16 mode ForwardTransformer.forward runs ONE autograd node, TransformerFn, with a backward of its own
(addln_bwd(own_dres=True), convbias_bwd / mha_bwd(dx_into=...): the residual joins as accumulate epilogues of the
data-gradient GEMMs), and at head width 64 / 128 that node hands all its FFTBlocks to ONE C call each way
(blocks_fwd_composite / blocks_bwd_composite -> csrc/ft_fft_block.hip: hand-carved arenas, block i+1's input aliased to
block i's y2, dx aliased to d_h, weight gradients behind four forks per block, eight column sums in one ft_colsum_batch,
ft_conv1d_bwd_data_relu).  This is what bench.py's variants.fastpitch_bf16_train runs.  Three routes of the same module:

  layer      FT_TRANSFORMER_NODE=0: PosEncFn / MHAFn / AddLayerNormFn / ConvBiasFn, the nodes the fp32 suite pins
  loop       FT_TRANSFORMER_NODE=1 FT_FFT_COMPOSITE=0: TransformerFn's Python loop
  composite  the bf16 default (composite_ok(d, heads) is asserted, so that loop is never compared with loop)

Part 1: one ForwardTransformer alone (tests/transformer_cases.py), loss (y * w).sum() over all rows, against
oracle.fp_oracle.forward_transformer in float64 and route against route, without dropout and with dropout 0.1.  Part 2: a small FastPitch whose five stacks all
qualify for the composite, under TrainStep (gradient sink + weight-gradient side stream: the branch the benchmark runs) and
under a plain backward.  Part 3: the pieces only this path uses, alone, in fp32 mode against float64.

Launch by launch (read off fastpitch.py and csrc/ft_fft_block.hip), the three routes issue the same kernels on the same
operands in the same order, with these differences, none of which changes a bit:
  * ReLU gradient of conv1: layer and loop run conv2's data-gradient GEMM, then ft_relu_bwd (dx = y > 0 ? dy : 0) as a pass
    of its own; the composite applies the same select in that GEMM's epilogue (ft_conv1d_bwd_data_relu; the mask does not
    enter the kernel choice of ft_launch_gemm_rows).  A select is exact.
  * the two residual joins: the layer route lets autograd add the two gradients of a tensor with two consumers (a + b);
    loop and composite pass the first as the `accumulate` operand of the GEMM that produces the second (epilogue
    v = acc; v += *c).  One fp32 addition of the same two numbers either way.
  * without dropout the layer route returns LayerNorm's dx for both branch and residual; loop and composite have the
    kernel store it twice (own_dres).
  * column sums: one ft_colsum / ft_colsum2 call each against ft_colsum_batch, which keeps every sum's chunking
    (test_batched_column_sums_are_bit_identical_to_one_call_each).
  * the composite reads its operands from arenas (16-byte aligned sub-buffers, so the GEMMs' 16-byte-load paths are the
    same) and, under TrainStep, runs weight gradients and sums on the side stream.
So rule (d) is torch.equal for every tensor, between all three routes, with and without dropout, and under TrainStep.

Observed on the MI355X (err = max|got - float64| / max(1, max|float64|); the three routes were bit-identical in every tensor
of every case, so loop and composite show the layer route's figures and the worst err / e_layer is 1.000 throughout):

  case                    fp32 loop, worst   bf16 e_layer: y    dx         largest gradient (tensor)
  hd64_T70_2layers        5.5e-6 (pe scale)  4.5e-3             7.2e-2     3.2e-1 (pos_encoder.scale)
  hd128_T129_k3k3         6.0e-7             2.8e-3             9.1e-2     1.0e-1 (layers.0.conv1.weight)
  hd64_T7_nomask          6.9e-7             3.3e-3             5.7e-2     3.6e-1 (layers.0.conv1.weight)
  hd128_T841_wide_tiles   1.2e-6             4.0e-3             4.7e-2     6.6e-2 (pos_encoder.scale)

With dropout 0.1 (training mode; the float64 reference gets the masks rebuilt on the CPU by tests/dropout_cpu.py, nothing of
them comes from the code under test), same columns, loop = layer in fp32 and all three routes bit-identical in bf16:

  hd64_T70_2layers        8.6e-7 (y)         4.8e-3             5.9e-2     1.3e-1 (layers.1.conv1.weight)
  hd128_T129_k3k3         7.0e-7             2.6e-3             1.1e-1     1.4e-1 (layers.0.conv1.weight)

The bf16 output sits at a few 1e-3, inside tol_mel.  The bf16 GRADIENTS of this loss are 5-10 % of their range away from
float64 on every route alike, and two kinds of tensor more: pos_encoder.scale is ONE sum over all B * T * d products with
heavy cancellation (-17.6 out of sum|terms| = 9494 in the first case; 5.6 is 6e-4 of that, and the fp32 route shows the same
7x against its neighbours); conv1's gradients are consistent with conv1's ReLU mask flipping wherever bf16 moves an h1
entry across zero, which a 7-row case does not average out.  So rule (c) alone, 2 * e_layer, would be a loose bar for
gradients; the bit-equal comparison of rule (d) is the one that holds the pointers, and the fp32 loop run is the one that
holds the arithmetic.
Part 2: loss 10.48836 (oracle 10.48756), grad_norm 8.8699 (8.8680); per-parameter e_layer from 1.6e-5 to 2.3e-3
(lin.weight), composite identical.  Part 3, observed / bound: conv1d_bwd_data_relu 0.02 / 0.07 / 0.38 (fp32) and 0.01 /
0.05 / 0.05 (bf16) for the three shapes; addln_bwd at most 0.028; convbias_bwd dx_into 0.04 / 0.17 / 0.06; mha_bwd dx_into
0.006 / 0.013.  The composite of the last case launched {'rows_b3_64': 7, 'rows_b3p': 1, 'tn_b3_64': 4}.
"""
import math

import pytest
import torch

from helpers import TRAIN_CFG, TINY_FP, maxdiff, rel_err
from transformer_cases import CASES, err, inputs, reference64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROUTES = ('layer', 'loop', 'composite')


def _set_route(mp, route):
    mp.delenv('FT_ATTN_FUSED', raising=False)
    if route == 'layer':
        mp.setenv('FT_TRANSFORMER_NODE', '0')
        mp.delenv('FT_FFT_COMPOSITE', raising=False)
    elif route == 'loop':
        mp.setenv('FT_TRANSFORMER_NODE', '1')
        mp.setenv('FT_FFT_COMPOSITE', '0')
    else:
        assert route == 'composite'
        mp.delenv('FT_TRANSFORMER_NODE', raising=False)
        mp.delenv('FT_FFT_COMPOSITE', raising=False)


def _replay_seed_stream(seed: int) -> None:
    """base._seed() re-bases its stream (from torch's host RNG) when it finds a torch seed different from the one it saw
    last: park it on another seed, then install `seed` -- the next forward draws the same dropout seeds every time.  Nothing
    may draw from torch's global RNG between this call and the forward."""
    from forwardtacotron_amd import base
    torch.manual_seed(seed + 1)
    base._seed()
    torch.manual_seed(seed)


_RUNS = {}


def _run(mp, name, mode, route, p=0.0, cached=True):
    """one forward + backward of the case's ForwardTransformer -> {'y', 'dx', <parameter name>: grad} on the CPU, plus
    '_variants': the GEMM variants launched meanwhile"""
    from forwardtacotron_amd import hip as H
    from forwardtacotron_amd import ops
    from forwardtacotron_amd.fastpitch import ForwardTransformer, composite_ok
    key = (name, mode, route, p)
    if cached and key in _RUNS:
        return _RUNS[key]
    c = CASES[name]
    P, x, pad, w = inputs(name)
    m = ForwardTransformer(c['d'], c['f'], c['layers'], c['nh'], c['k1'], c['k2'], dropout=p)
    m.load_state_dict(P)
    m = m.cuda().train()
    xg = x.cuda().requires_grad_(True)
    padg = pad.cuda() if pad is not None else None
    _set_route(mp, route)
    assert ops._SINK is None                    # part 1 is the one-stream branch of blocks_bwd_composite
    _replay_seed_stream(4242)
    with H.gemm_precision(mode):
        if route == 'composite':
            assert mode == 'bf16' and composite_ok(c['d'], c['nh']), 'the composite must be live, or loop meets loop'
        elif route == 'loop':
            assert not composite_ok(c['d'], c['nh'])
        v0 = H.gemm_variant_counts()
        y = m(xg, padg)
        (y * w.cuda()).sum().backward()
        torch.cuda.synchronize()
        v1 = H.gemm_variant_counts()
    out = {'y': y.detach().cpu(), 'dx': xg.grad.cpu()}
    out.update({k: q.grad.cpu() for k, q in m.named_parameters()})
    assert set(out) == set(reference64(name))
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), (key, k)
    out['_variants'] = {k: v1[k] - v0[k] for k in v1 if v1[k] != v0[k]}
    if cached:
        _RUNS[key] = out
    return out


def _tensors(res):
    return [k for k in res if not k.startswith('_')]


def _assert_bitwise(a, b, what):
    bad = [(k, maxdiff(a[k], b[k])) for k in _tensors(a) if not torch.equal(a[k], b[k])]
    assert not bad, (what, bad)


# ---------------------------------------------------------------------------------------------------
# 1. the three routes of one ForwardTransformer
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_fp32_loop_route_vs_float64(monkeypatch, name):
    """(a) fp32 mode: TransformerFn's own backward arithmetic (own_dres, dx_into, posenc_bwd_scale) with no bf16 noise in
    the way, held to the bars test_fastpitch_wide_vs_oracle holds the per-layer route to: 1e-4 on the output, 2e-4 *
    max(1, |g|max) on every gradient.  The layer route runs beside it; same kernels, so the two are also bit-equal."""
    ref = reference64(name)
    loop = _run(monkeypatch, name, 'fp32', 'loop')
    layer = _run(monkeypatch, name, 'fp32', 'layer')
    worst = 0.0
    for k in _tensors(loop):
        e_loop, e_layer = err(loop[k], ref[k]), err(layer[k], ref[k])
        worst = max(worst, e_loop)
        print(f'fp32 {name} {k:40s} loop {e_loop:.3e}  layer {e_layer:.3e}')
    print(f'fp32 {name} worst loop error {worst:.3e}')
    for k in _tensors(loop):
        assert err(loop[k], ref[k]) < (1e-4 if k == 'y' else 2e-4), (k, err(loop[k], ref[k]))
    _assert_bitwise(loop, layer, 'fp32 loop vs layer')


@pytest.mark.parametrize('name', list(CASES))
def test_bf16_routes_vs_float64_and_the_layer_yardstick(monkeypatch, name):
    """(b), (c) bf16 mode, dropout 0.  e_layer[k] = error of the layer route (the code the fp32 suite pins; the yardstick,
    not under test) against float64; loop and composite must satisfy err[k] <= 2 * e_layer[k] + 1e-6 (the bar of
    test_gpu_multi_fastpitch_generate_batch.py: same operand rounding, another summation order at most).  The yardstick
    itself must be a bf16-sized number: on the output, above fp32 noise and inside the 8e-2 the bf16 model tests state as
    tol_mel (a tolerance on a forward output; the suite states none for a bf16 gradient but grad_norm within 3 %).  The
    gradients' yardsticks are printed, not bounded: see the module docstring for what they came to."""
    ref = reference64(name)
    res = {r: _run(monkeypatch, name, 'bf16', r) for r in ROUTES}
    e_layer = {k: err(res['layer'][k], ref[k]) for k in _tensors(ref)}
    worst_ratio = 0.0
    for k in _tensors(ref):
        es = {r: err(res[r][k], ref[k]) for r in ('loop', 'composite')}
        ratio = max(es.values()) / e_layer[k] if e_layer[k] > 0 else float('inf' if max(es.values()) > 0 else 0)
        worst_ratio = max(worst_ratio, ratio)
        print(f'bf16 {name} {k:40s} e_layer {e_layer[k]:.3e}  loop {es["loop"]:.3e}  composite {es["composite"]:.3e}'
              f'  ratio {ratio:.3f}')
    print(f'bf16 {name} e_layer[y] {e_layer["y"]:.3e}  largest gradient e_layer {max(e_layer.values()):.3e}  '
          f'worst err / e_layer {worst_ratio:.3f}')
    assert 1e-5 < e_layer['y'] < 8e-2, e_layer['y']
    for k in _tensors(ref):
        for r in ('loop', 'composite'):
            e = err(res[r][k], ref[k])
            assert e <= 2 * e_layer[k] + 1e-6, (r, k, e, e_layer[k])


@pytest.mark.parametrize('name', list(CASES))
def test_bf16_routes_are_bit_identical(monkeypatch, name):
    """(d) route against route, directly: where a wrong pointer shows at full size, with no bf16 slack.  The module
    docstring lists every launch that differs between the routes; none of them changes a bit, so every tensor is
    torch.equal between composite and loop and between loop and layer."""
    res = {r: _run(monkeypatch, name, 'bf16', r) for r in ROUTES}
    _assert_bitwise(res['composite'], res['loop'], 'composite vs loop')
    _assert_bitwise(res['loop'], res['layer'], 'loop vs layer')


def test_wide_tile_gemms_ran_inside_the_composite(monkeypatch):
    """The last case's row count is above the launcher's tile switch (csrc/ft_gemm_plan.h: tiles_big = at least 192
    128x128 tiles, M and N above 64): the in-projection [B*T, d] x [d, 3d] has ceil(B*T / 128) * ceil(3d / 128) tiles, so
    with d = 256 it switches at B*T > 31 * 128 = 3968 rows; 5 * 841 = 4205 cross it, B did not have to be raised.  In bf16
    mode the 128x128 tile is the pipelined kernel ('rows_b3p'), which nothing else in the case launches: its counter moves
    by exactly one launch per block, inside ft_fft_blocks_fwd.  (The other GEMMs of the case have N = 256: 66 tiles, the
    64x64 kernel, like the narrower cases -- both tile sizes run inside one composite call.)"""
    name = 'hd128_T841_wide_tiles'
    c = CASES[name]
    rows = c['B'] * c['T']
    tiles = math.ceil(rows / 128) * math.ceil(3 * c['d'] / 128)
    assert tiles >= 192 and (math.ceil(rows / 128) - 2) * math.ceil(3 * c['d'] / 128) < 192, 'just above the switch'
    comp = _run(monkeypatch, name, 'bf16', 'composite')['_variants']
    print('GEMM variants inside the composite:', comp)
    assert comp.get('rows_b3p', 0) == c['layers'], comp
    assert comp.get('rows_b3_64', 0) > 0, comp
    small = _run(monkeypatch, 'hd64_T70_2layers', 'bf16', 'composite')['_variants']
    assert small.get('rows_b3p', 0) == 0, small


@pytest.mark.parametrize('name', ['hd64_T70_2layers', 'hd128_T129_k3k3'])
def test_bf16_routes_with_dropout_are_bit_identical_and_reproducible(monkeypatch, name):
    """(e), (f) dropout 0.1 in training mode: positional-encoding dropout, attention dropout inside the fused kernel and
    the two residual dropouts fused into the LayerNorms, all from the library's counter-based mask.  This test compares
    route with route; the float64 reference with the same masks, rebuilt on the CPU, is in the two dropout tests below.
    The three routes draw the same seeds in the same order (replayed through base._seed()'s documented re-basing), so rule
    (d) applies: bit-equal.  The masks were really on (the output differs from the dropout-0 output), and a second
    composite run with the same seeds reproduces every gradient bit for bit (no atomics on the path)."""
    res = {r: _run(monkeypatch, name, 'bf16', r, p=0.1) for r in ROUTES}
    clean = _run(monkeypatch, name, 'bf16', 'composite')
    for r in ROUTES:
        assert maxdiff(res[r]['y'], clean['y']) > 1e-2, r
    _assert_bitwise(res['composite'], res['loop'], 'dropout: composite vs loop')
    _assert_bitwise(res['loop'], res['layer'], 'dropout: loop vs layer')
    again = _run(monkeypatch, name, 'bf16', 'composite', p=0.1, cached=False)
    _assert_bitwise(again, res['composite'], 'composite, second run with the same seeds')


DROPOUT_CASES = ['hd64_T70_2layers', 'hd128_T129_k3k3']


@pytest.mark.parametrize('name', DROPOUT_CASES)
def test_fp32_routes_with_dropout_vs_float64(monkeypatch, name):
    """dropout 0.1, fp32 mode: loop and layer route against the float64 oracle run with THE SAME masks, rebuilt on the CPU
    (tests/dropout_cpu.py: the restated mixer, the restated seed stream of torch.manual_seed(4242), the documented draw order
    pe, then per layer attention, norm1, norm2, and each site's index layout) -- nothing of the mask comes from the code
    under test.  The bars of test_fp32_loop_route_vs_float64: 1e-4 on y, 2e-4 on every gradient.  A wrong seed order, a
    site indexing another layout, a backward that rebuilds another mask than its forward or a keep scale other than
    1/(1-p) is an O(0.1) error here."""
    ref = reference64(name, 0.1)
    assert err(ref['y'], reference64(name)['y']) > 1e-2                     # the masks are on in the reference
    res = {r: _run(monkeypatch, name, 'fp32', r, p=0.1) for r in ('loop', 'layer')}
    for r, out in res.items():
        worst = max(err(out[k], ref[k]) for k in _tensors(out))
        print(f'fp32 p 0.1 {name} {r}: y {err(out["y"], ref["y"]):.3e}  worst {worst:.3e}')
    for r, out in res.items():
        for k in _tensors(out):
            assert err(out[k], ref[k]) < (1e-4 if k == 'y' else 2e-4), (r, k, err(out[k], ref[k]))


@pytest.mark.parametrize('name', DROPOUT_CASES)
def test_bf16_routes_with_dropout_vs_float64_and_the_layer_yardstick(monkeypatch, name):
    """dropout 0.1, bf16 mode, against the float64 oracle with the CPU-built masks: loop and composite within
    2 * e_layer + 1e-6, e_layer the layer route's own error at p = 0.1, and 1e-5 < e_layer[y] < 8e-2 as at p = 0 -- a
    mask that differed from the reference's anywhere would put e_layer[y] at O(0.1) or above."""
    ref = reference64(name, 0.1)
    res = {r: _run(monkeypatch, name, 'bf16', r, p=0.1) for r in ROUTES}
    e_layer = {k: err(res['layer'][k], ref[k]) for k in _tensors(ref)}
    print(f'bf16 p 0.1 {name} e_layer[y] {e_layer["y"]:.3e}  e_layer[dx] {e_layer["dx"]:.3e}  largest gradient e_layer '
          f'{max(e_layer.values()):.3e} ({max(e_layer, key=e_layer.get)})')
    assert 1e-5 < e_layer['y'] < 8e-2, e_layer['y']
    for k in _tensors(ref):
        for r in ('loop', 'composite'):
            e = err(res[r][k], ref[k])
            assert e <= 2 * e_layer[k] + 1e-6, (r, k, e, e_layer[k])


# ---------------------------------------------------------------------------------------------------
# 2. the same comparison with the gradient sink and its side stream on (TrainStep)
# ---------------------------------------------------------------------------------------------------
SMALL_FP = dict(TINY_FP,
                durpred_d_model=64, durpred_n_heads=1, durpred_layers=1, durpred_d_fft=96,
                pitch_d_model=64, pitch_n_heads=1, pitch_layers=2, pitch_d_fft=80,
                energy_d_model=64, energy_n_heads=1, energy_layers=1, energy_d_fft=64,
                d_model=128, conv1_kernel=9, conv2_kernel=1,
                prenet_layers=2, prenet_heads=2, prenet_fft=192, postnet_layers=2, postnet_heads=2, postnet_fft=160,
                n_mels=20)


@pytest.fixture(scope='module')
def small_fp():
    """-> (initial state dict, batch, oracle.fp_oracle.train_step's info) of the small all-composite FastPitch"""
    from oracle import fp_oracle as FP
    from oracle.ft_oracle import synthetic_batch
    from forwardtacotron_amd.fastpitch import FastPitch
    torch.manual_seed(23)
    m = FastPitch(**SMALL_FP)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    batch = synthetic_batch(B=4, Tmax=23, n_mels=20, max_dur=6, seed=5)
    _, _, info = FP.train_step(P, {}, batch, SMALL_FP, TRAIN_CFG, 1e-3, 1)
    return P, batch, info


def _fresh_fp(P):
    from forwardtacotron_amd.fastpitch import FastPitch
    m = FastPitch(**SMALL_FP)
    m.load_state_dict(P)
    m = m.cuda()
    m.matmul_dtype = 'bf16'
    return m


def _train_step(mp, P, batch, route):
    from forwardtacotron_amd.trainer import TrainStep
    _set_route(mp, route)
    m = _fresh_fp(P)
    ts = TrainStep(m, lr=1e-3, train_cfg=TRAIN_CFG)
    assert ts.sink.stream is not None
    out = ts.step({k: v.clone().cuda() for k, v in batch.items()})
    ts.check()
    torch.cuda.synchronize()
    res = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
    res['loss'] = out['loss'].detach().cpu().clone()
    res['grad_norm'] = out['grad_norm'].detach().cpu().clone()
    ts.close()
    return res


def _plain_backward(mp, P, batch):
    from forwardtacotron_amd import hip as H
    from forwardtacotron_amd import ops
    _set_route(mp, 'composite')
    m = _fresh_fp(P).train()
    b = {k: v.clone().cuda() for k, v in batch.items()}
    pitch_t, energy_t = b['pitch'].clone(), b['energy'].clone()
    c = TRAIN_CFG
    assert ops._SINK is None
    with H.gemm_precision('bf16'):              # TrainStep holds the mode over forward AND backward
        pred = m(b)
        side = c['dur_loss_factor'] * ops.masked_l1(pred['dur'].unsqueeze(1), b['dur'].unsqueeze(1), b['x_len']) \
            + c['pitch_loss_factor'] * ops.masked_l1(pred['pitch'], pitch_t.unsqueeze(1), b['x_len']) \
            + c['energy_loss_factor'] * ops.masked_l1(pred['energy'], energy_t.unsqueeze(1), b['x_len'])
        loss = ops.masked_l1(pred['mel'], b['mel'], b['mel_len']) + ops.masked_l1(pred['mel_post'], b['mel'], b['mel_len']) \
            + side                              # TrainStep.losses' order of additions
        loss.backward()
        torch.cuda.synchronize()
    res = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
    res['loss'] = loss.detach().cpu().clone()
    return res


def test_trainstep_routes_bit_identical_and_vs_oracle(monkeypatch, small_fp):
    """One TrainStep.step per route from identical weights (fresh model, fresh TrainStep): the composite then writes its
    gradients straight into the flat buffer's views and runs its weight-gradient GEMMs and column sums on the sink's side
    stream behind the follow() forks of ft_fft_blocks_bwd -- the branch the benchmark runs.  Rule (d): loss, grad_norm and
    every parameter's gradient are bit-equal between the routes, and the composite under TrainStep equals the composite
    under a plain loss.backward() with no sink (p.grad is compared as the step leaves it: TrainStep never scales the
    gradient buffer, the clip coefficient only enters ft_adam_step).  Against oracle.fp_oracle.train_step (fp32), per
    parameter, err_composite <= 2 * err_layer + 1e-6 with the layer route as yardstick."""
    from forwardtacotron_amd import hip as H
    from forwardtacotron_amd.fastpitch import composite_ok
    P, batch, info = small_fp
    with H.gemm_precision('bf16'):
        for d, nh in ((64, 1), (128, 2)):
            assert composite_ok(d, nh)
    res = {r: _train_step(monkeypatch, P, batch, r) for r in ROUTES}
    plain = _plain_backward(monkeypatch, P, batch)
    names = [k for k in res['layer'] if k not in ('loss', 'grad_norm')]
    assert set(names) == set(info['grads'])
    print(f"loss {float(res['composite']['loss']):.6f} (oracle {float(info['losses']['loss']):.6f})  grad_norm "
          f"{float(res['composite']['grad_norm']):.6f} (oracle {float(info['grad_norm']):.6f})")
    worst = 0.0
    for k in names:
        e_layer = err(res['layer'][k], info['grads'][k])
        e_comp = err(res['composite'][k], info['grads'][k])
        worst = max(worst, e_comp / e_layer if e_layer > 0 else 0.0)
        print(f'TrainStep {k:48s} e_layer {e_layer:.3e}  composite {e_comp:.3e}')
        assert e_comp <= 2 * e_layer + 1e-6, (k, e_comp, e_layer)
    print(f'TrainStep worst err_composite / err_layer {worst:.3f}')
    for a, b_ in (('composite', 'loop'), ('loop', 'layer')):
        bad = [(k, maxdiff(res[a][k], res[b_][k])) for k in res[a] if not torch.equal(res[a][k], res[b_][k])]
        assert not bad, (a, b_, bad)
    bad = [(k, maxdiff(plain[k], res['composite'][k])) for k in plain if not torch.equal(plain[k], res['composite'][k])]
    assert not bad, ('plain backward vs TrainStep', bad)


def test_composite_backward_keeps_every_side_stream_operand_alive(monkeypatch, small_fp):
    """Under TrainStep the composite's weight gradients run on the sink's side stream, and TransformerFn.backward drops
    the forward's state the moment blocks_bwd_composite returns.  Whatever those launches read must therefore sit in
    GradSink.keep until the step joins the side stream -- also block 0's input `h`, the operand of the LAST weight gradient
    issued (the in-projection's of block 0): a freed `h` is the main stream's to reuse while that GEMM still reads it, which
    showed as one wrong in_proj_weight gradient (5.9e-3 from the oracle instead of 3.5e-5) in
    test_trainstep_routes_bit_identical_and_vs_oracle, depending on what the allocator had cached from earlier tests.  Host-side and
    deterministic: the addresses held by the sink right after each composite backward."""
    from forwardtacotron_amd import fastpitch as F
    from forwardtacotron_amd import ops
    P, batch, _ = small_fp
    real, seen = F.blocks_bwd_composite, []

    def tensors(x):
        if torch.is_tensor(x):
            yield x
        elif isinstance(x, (list, tuple)):
            for y in x:
                yield from tensors(y)

    def spy(state, dy, params):
        out = real(state, dy, params)
        sink = ops._SINK
        assert sink is not None and sink.stream is not None
        held = {t.data_ptr() for t in tensors(sink.keep)}
        seen.append(state['h'].data_ptr() in held and all(a.data_ptr() in held for a in state['arenas'])
                    and dy.data_ptr() in held)
        return out

    monkeypatch.setattr(F, 'blocks_bwd_composite', spy)
    _train_step(monkeypatch, P, batch, 'composite')
    assert len(seen) == 5 and all(seen), seen               # dur, pitch, energy, prenet, postnet


# ---------------------------------------------------------------------------------------------------
# 3. the pieces only this path uses, alone, against float64
# ---------------------------------------------------------------------------------------------------
def _conv_dx64(dy, w, k, T):
    """float64 data gradient of nn.Conv1d(Cin, Cout, k, padding=k//2) on channels-last dy [B,T,Cout] -> [B,T,Cin]"""
    x = torch.zeros(dy.shape[0], w.shape[1], T, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv1d(x, w.double(), padding=k // 2)
    (y * dy.double().transpose(1, 2)).sum().backward()
    return x.grad.transpose(1, 2).contiguous()


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,T,Cin,Cout,k', [(2, 9, 8, 12, 1), (3, 37, 24, 16, 3), (2, 130, 192, 128, 9)])
def test_conv1d_bwd_data_relu_vs_float64(B, T, Cin, Cout, k, mode):
    """ft_conv1d_bwd_data_relu (conv2's data gradient through conv1's ReLU, the mask in the GEMM's epilogue) against the
    float64 data gradient times (h1 > 0).  h1 carries planted exact zeros, a negative zero and negative values (they must
    mask: the reference's ReLU gradient is 0 at 0 -- the result is EXACTLY 0.0 there) and a tiny positive value (it must
    pass).  fp32 mode: the 3e-6 relative bar test_conv1d_fwd_bwd holds the unmasked data gradient to.  bf16 mode: operands
    rounded to bf16 beforehand, against float64 of the rounded operands, the bar of
    test_bf16_gemm_rounds_operands_and_accumulates_in_fp32 (2e-6 * scale * max(1, sqrt(K / 64)), K = Cout * k the
    contraction length)."""
    from forwardtacotron_amd import hip as H
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + k)
    dy = torch.randn(B, T, Cout, generator=g)
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cout * k)
    h1 = torch.randn(B, T, Cin, generator=g)
    n = h1.numel()
    flat = h1.view(-1)
    zeros, negz, negs, tiny = [0, n // 3, n - 1], [1, n // 2], [2, n // 2 + 1, n - 2], [3, n // 2 + 2]
    flat[zeros], flat[negz], flat[negs], flat[tiny] = 0.0, -0.0, -0.5, 1e-30
    if mode == 'bf16':
        dy, w = dy.bfloat16().float(), w.bfloat16().float()
    full = _conv_dx64(dy, w, k, T)
    ref = full * (h1 > 0).double()
    with H.gemm_precision(mode):
        got = H.conv1d_bwd_data_relu(dy.cuda(), w.cuda(), h1.cuda()).cpu()
    scale = float(full.abs().max())
    bound = 3e-6 * scale if mode == 'fp32' else 2e-6 * scale * max(1.0, math.sqrt(Cout * k / 64))
    d = float((got.double() - ref).abs().max())
    print(f'conv1d_bwd_data_relu {mode} {(B, T, Cin, Cout, k)}: observed / bound = {d / bound:.3f}')
    assert d <= bound, (d, bound)
    gf = got.view(-1)
    assert bool((gf[zeros + negz + negs] == 0.0).all()) and bool((got[h1 <= 0] == 0.0).all())
    assert bool((full.view(-1)[zeros + negz + negs].abs() > 0).all())       # (there was something to mask)
    assert bool((gf[tiny].double() - full.view(-1)[tiny]).abs().max() <= bound) and bool((gf[tiny] != 0).all())
    assert float((h1 > 0).float().mean()) > 0.3 and float((h1 <= 0).float().mean()) > 0.3


@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('rows,D', [(27, 16), (65, 130), (300, 256)])
def test_addln_bwd_with_its_own_residual_gradient_vs_float64(rows, D, p):
    """addln_bwd(..., own_dres=True): the gradients of y = LayerNorm(x + dropout_p(res)) wrt x and wrt res, the second in a
    buffer of its own (the composite accumulates conv1's data gradient into the first while conv2's weight gradient still
    reads the second on the other stream).  The dropout mask is the library's counter-based one, rebuilt through H.dropout
    on ones.  Bound per element, from the kernel's arithmetic (two sums of D fp32 terms per row, on a normalised row whose
    statistics carry the error of two more): (2 D + 32) u rstd (|a| + mean|a| + |xhat| mean|a xhat|), a = gamma dy."""
    from forwardtacotron_amd import hip as H
    from forwardtacotron_amd.fastpitch import addln_bwd, addln_fwd
    g = torch.Generator().manual_seed(rows * 5 + D)
    x, res, dy = (torch.randn(rows, D, generator=g) for _ in range(3))
    gamma = 1 + 0.2 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    seed, eps = 20240607, 1e-5
    keep = torch.ones(rows, D, dtype=torch.float64)
    if p > 0:
        keep = (H.dropout(torch.ones(rows * D, device='cuda'), p, seed) > 0).double().cpu().reshape(rows, D)
        assert abs(float(keep.mean()) - (1 - p)) < 0.1
    x64, r64 = x.double().requires_grad_(True), res.double().requires_grad_(True)
    s = x64 + r64 * keep / (1 - p)
    y64 = torch.nn.functional.layer_norm(s, (D,), gamma.double(), beta.double(), eps)
    (y64 * dy.double()).sum().backward()
    xd, rd, dyd, gd, bd = (t.cuda() for t in (x, res, dy, gamma, beta))
    y, tape = addln_fwd(xd, rd, gd, bd, eps, p, seed)
    dx, dres, dg, db = addln_bwd(tape, dyd, gd, bd, own_dres=True)
    torch.cuda.synchronize()
    assert maxdiff(y.cpu(), y64.detach()) < 5e-6                           # (test_add_layernorm's forward bar)
    sd = s.detach()
    rstd = 1.0 / torch.sqrt(sd.var(-1, unbiased=False, keepdim=True) + eps)
    xhat = (sd - sd.mean(-1, keepdim=True)) * rstd
    a = gamma.double() * dy.double()
    bound = (2 * D + 32) * U * rstd * (a.abs() + a.abs().mean(-1, keepdim=True)
                                       + xhat.abs() * (a * xhat).abs().mean(-1, keepdim=True))
    for name, got, ref, b_ in (('d_x', dx, x64.grad, bound), ('d_res', dres, r64.grad, bound * keep / (1 - p))):
        d = (got.cpu().double() - ref).abs()
        live = b_ > 0
        print(f'addln_bwd own_dres rows {rows} D {D} p {p} {name}: observed / bound = '
              f'{float((d[live] / b_[live]).max()):.3f}')
        assert bool((d <= b_).all()), (name, float(d.max()))
    if p > 0:
        assert bool((dres.cpu()[keep == 0] == 0.0).all()) and float((keep == 0).double().mean()) > 0.5 * p
    else:
        assert torch.equal(dres, dx)
    # a buffer of its own: neither the input gradient's nor the upstream gradient's memory
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * 4) for t in (dres, dx, dyd)]
    assert spans[0][1] <= spans[1][0] or spans[1][1] <= spans[0][0]
    assert spans[0][1] <= spans[2][0] or spans[2][1] <= spans[0][0]
    assert tuple(dg.shape) == (D,) and tuple(db.shape) == (D,)


@pytest.mark.parametrize('B,T,Cin,Cout,k,relu', [(2, 9, 8, 10, 3, True), (2, 70, 24, 40, 9, False),
                                                 (3, 50, 32, 48, 1, True)])
def test_convbias_bwd_accumulates_into_an_existing_gradient(B, T, Cin, Cout, k, relu):
    """convbias_bwd(..., dx_into=buf): buf (random beforehand) becomes buf + dx IN PLACE, against float64.  Cout = 10 takes
    the [K][N] weight form, the others the transposed one; the last two have more than 128 rows.  Bound: the 3e-6 relative
    bar of test_conv1d_fwd_bwd on the product plus one rounding of the sum."""
    from forwardtacotron_amd.fastpitch import convbias_bwd, convbias_fwd
    g = torch.Generator().manual_seed(T * 3 + Cout)
    x, dy = torch.randn(B, T, Cin, generator=g), torch.randn(B, T, Cout, generator=g)
    buf0 = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)
    b = 0.1 * torch.randn(Cout, generator=g)
    x64 = x.double().requires_grad_(True)
    y64 = torch.nn.functional.conv1d(x64.transpose(1, 2), w.double(), b.double(), padding=k // 2).transpose(1, 2)
    if relu:
        y64 = torch.relu(y64)
    (y64 * dy.double()).sum().backward()
    y, tape = convbias_fwd(x.cuda(), w.cuda(), b.cuda(), relu)
    assert rel_err(y, y64.detach()) < 3e-6
    buf = buf0.clone().cuda()
    ptr = buf.data_ptr()
    dx, dw, db = convbias_bwd(tape, dy.cuda(), w.cuda(), b.cuda(), dx_into=buf)
    assert dx is buf and buf.data_ptr() == ptr
    ref = buf0.double() + x64.grad
    bound = 3e-6 * float(x64.grad.abs().max()) + U * float(ref.abs().max())
    d = maxdiff(buf.cpu(), ref)
    print(f'convbias_bwd dx_into {(B, T, Cin, Cout, k, relu)}: observed / bound = {d / bound:.3f}')
    assert d <= bound, (d, bound)
    assert maxdiff(buf.cpu(), buf0) > 0.1                                   # (it did add something)


@pytest.mark.parametrize('B,T,d,nh', [(2, 9, 16, 2), (2, 70, 64, 2)])
def test_mha_bwd_accumulates_into_an_existing_gradient(B, T, d, nh):
    """mha_bwd(..., dx_into=buf) in fp32 mode: buf becomes buf + dx in place (the in-projection's data-gradient GEMM with
    the accumulate epilogue), against the float64 attention of oracle.fp_oracle.mha with a ragged key mask.  Bound: the
    5e-5 bar test_attention_matches_torch_mha holds dx to (scaled by max(1, |dx|max)) plus one rounding of the sum."""
    from oracle import fp_oracle as FP
    from forwardtacotron_amd.fastpitch import mha_bwd, mha_fwd
    g = torch.Generator().manual_seed(B * 100 + T)
    x, dout, buf0 = (torch.randn(B, T, d, generator=g) for _ in range(3))
    P = {'in_proj_weight': torch.randn(3 * d, d, generator=g) / math.sqrt(d),
         'in_proj_bias': 0.2 * torch.randn(3 * d, generator=g),
         'out_proj.weight': torch.randn(d, d, generator=g) / math.sqrt(d),
         'out_proj.bias': 0.2 * torch.randn(d, generator=g)}
    lens = torch.tensor([T, T // 2 + 1])
    pad = torch.arange(T)[None, :] >= lens[:, None]
    x64 = x.double().requires_grad_(True)
    y64 = FP.mha(x64, pad, {k: v.double() for k, v in P.items()}, '', nh)
    (y64 * dout.double()).sum().backward()
    ps = [P[k].cuda() for k in ('in_proj_weight', 'in_proj_bias', 'out_proj.weight', 'out_proj.bias')]
    y, tape = mha_fwd(x.cuda(), pad.to(torch.uint8).cuda(), *ps, nh, 0.0, 0)
    assert not tape['fused'] and maxdiff(y.cpu(), y64.detach()) < 2e-5
    buf = buf0.clone().cuda()
    ptr = buf.data_ptr()
    dx = mha_bwd(tape, dout.cuda(), *ps, dx_into=buf)[0]
    assert dx is buf and buf.data_ptr() == ptr
    ref = buf0.double() + x64.grad
    bound = 5e-5 * max(1.0, float(x64.grad.abs().max())) + U * float(ref.abs().max())
    dd = maxdiff(buf.cpu(), ref)
    print(f'mha_bwd dx_into {(B, T, d, nh)}: observed / bound = {dd / bound:.3f}')
    assert dd <= bound, (dd, bound)
    assert maxdiff(buf.cpu(), buf0) > 0.1
