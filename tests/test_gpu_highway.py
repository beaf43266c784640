"""GPU: the HighwayNetwork kernels, each alone through the C ABI, element by element against tests/highway_cpu.py
(float64 numpy; proven by tests/test_highway_cpu.py, which also holds the fixtures' properties):

  ft_highway_pack      ft_highway_pack_kernel, bit for bit
  ft_highway_fwd       ft_highway_epilogue mode 1: the LDS form (TN == 1) on ft_gemm_rows_kernel's 64 tile and on the
                       64-tile bf16 kernel, the one-lane form (TN == 2) on the pipelined kernel and on the f32 128 tile
  ft_highway_gate_*    ft_highway_fwd_kernel / ft_highway_bwd_kernel
  ft_highway_bwd_data  the chained data gradient, plain and with the mode-2 epilogue, NT and NN, fp32 and bf16 mode
  ops.highway_stack    as a composition: bit-equal to the chain of kernel calls, parameter gradients from the chain's
                       own d12 and x

Every kernel is tested from its own fp32 inputs (the gate from the pre-activations the device stored, the backward from
a given x12), so the reference never re-makes a ReLU decision: EVERY element is held to an a-priori rounding bound
(highway_cpu.gate / gate_bwd / bwd_data_below; lens_cpu.conv_f32_bound / conv_b3_bound for the products) -- no quantile,
no excluded rows.  Each case asserts the launch-variant delta of the one kernel it is about, prints its worst
|err| / bound (pytest -s), carves every operand from a NaN-filled buffer and gives every output NaN guard rows that must
still be NaN afterwards; every result must be finite.

Not covered: rows_b3_128 and rows_f32_128_nt_fast under the highway epilogues.  They are reachable only with
FT_GEMM_PIPE=0 / FT_GEMM_B3=0, which the library reads once per process."""
import functools

import numpy as np
import pytest
import torch

import highway_cpu as R
from helpers import rel_err
from test_gpu_gemm_edges import Out, _call, counted, poison, ptr

pytestmark = pytest.mark.gpu

f32 = np.float32
SEEDS = {name: 100 + i for i, name in enumerate(R.SHAPES)}


@pytest.fixture(scope='module')
def H():
    from forwardtacotron_amd import hip
    assert torch.cuda.is_available()
    return hip


def op(a, ld=None, mis=0):
    """numpy operand (a vector as one row) -> device view inside a NaN-filled buffer"""
    a = np.ascontiguousarray(a, dtype=f32)
    return poison(torch.from_numpy(a[None] if a.ndim == 1 else a), ld, mis)


def fetch(out):
    """Out -> float32 numpy, after the guard and finiteness checks"""
    return out.check().numpy().astype(f32)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def worst(got, want, bound, what):
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), what
    ratio = np.abs(got - want) / bound
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f'    {what}: worst |err| / bound = {float(ratio[at]):.3f}')
    assert ratio[at] <= 1.0, (what, float(ratio[at]), at, float(got[at]), float(want[at]))


def wide(g, rows, cols, spread):
    """values whose rows span a wide dynamic range"""
    return (g.standard_normal((rows, cols)) * np.exp(spread * g.standard_normal((rows, 1)))).astype(f32)


class bf16_mode:
    """hip.gemm_precision('bf16') if on, and the proof that the mode is restored afterwards"""

    def __init__(self, H, on):
        self.H, self.on = H, on

    def __enter__(self):
        assert self.H.gemm_precision_mode() == 'fp32'
        if self.on:
            self.cm = self.H.gemm_precision('bf16')
            self.cm.__enter__()

    def __exit__(self, *exc):
        if self.on:
            self.cm.__exit__(*exc)
        assert self.H.gemm_precision_mode() == 'fp32'
        assert self.H.set_gemm_precision('fp32') == 'fp32', 'the library was left in bf16 mode'


# ---------------------------------------------------------------------------------------------------
# 1. ft_highway_pack
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [32, 96, 160])
def test_pack_is_the_32_row_interleave(H, C):
    g = np.random.default_rng(C)
    w1, w2 = g.standard_normal((C, C)).astype(f32), g.standard_normal((C, C)).astype(f32)
    w1d, w2d = op(w1), op(w2)
    out = Out(2 * C, C, flat=True)
    counted(H, {}, lambda: _call('ft_highway_pack', ptr(w1d), ptr(w2d), out.ptr, C, H._stream()))
    assert np.array_equal(bits(fetch(out)), bits(R.pack(w1, w2)))


def test_pack_refuses_a_width_that_is_no_multiple_of_32(H):
    from forwardtacotron_amd._lib import FtError
    C = 48
    w = op(np.ones((C, C)))
    out = Out(2 * C, C, flat=True)
    with pytest.raises(FtError, match='C % 32 == 0'):
        _call('ft_highway_pack', ptr(w), ptr(w), out.ptr, C, H._stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all()), 'refused, yet something was launched'


# ---------------------------------------------------------------------------------------------------
# 2. - 4. ft_highway_fwd: x12 against the float64 product (GEMM bound), out against the float64 gate of the device's
# own stored x12 (gate bound); save = False (x12 = nullptr, the eval path) bit-equal
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_ref(name, special, bf16):
    rows, C = R.SHAPES[name]
    x, w1, b1, w2, b2 = R.layer(rows, C, SEEDS[name], special)
    want12, mag = R.preact(x, w1, b1, w2, b2, bf16)
    return x, R.pack(w1, w2), b1, b2, want12, mag


def fused_fwd(H, xd, wd, b1d, b2d, rows, C, variant, save=True):
    out = Out(rows, C, flat=True)
    x12 = Out(rows, 2 * C, flat=True) if save else None
    counted(H, variant, lambda: _call('ft_highway_fwd', ptr(xd), ptr(wd), ptr(b1d), ptr(b2d), out.ptr,
                                      x12.ptr if save else None, rows, C, H._stream()))
    return out, x12


def check_fwd(H, name, variant, kernel, mis=0, special=False):
    rows, C = R.SHAPES[name]
    bf16 = kernel == 'bf16'
    x, w12i, b1, b2, want12, mag = fwd_ref(name, special, bf16)
    xd, wd, b1d, b2d = op(x, mis=mis), op(w12i), op(b1), op(b2)
    tag = f'fwd {name} {variant}' + (' special' if special else '')
    with bf16_mode(H, bf16):
        out, x12 = fused_fwd(H, xd, wd, b1d, b2d, rows, C, variant)
        out_nosave, _ = fused_fwd(H, xd, wd, b1d, b2d, rows, C, variant, save=False)
    got12, got = fetch(x12), fetch(out)
    worst(got12, want12, R.gemm_bound(mag, np.concatenate([b1, b2]), C, kernel), tag + ' x12')
    want, _, bound = R.gate(got12, x)
    worst(got, want, bound, tag + ' out')
    assert np.array_equal(bits(fetch(out_nosave)), bits(got)), 'save = False changed the output'
    return got12, got


FWD_F32 = [('tiny1', 'rows_f32_64_nt_fast', 'f32', 0), ('tiny77', 'rows_f32_64_nt_fast', 'f32', 0),
           ('edge64', 'rows_f32_64_nt_fast', 'f32', 0), ('small', 'rows_f32_64_nt_fast', 'f32', 0),
           ('big160', 'rows_b3p', 'b3', 0), ('big96', 'rows_b3p', 'b3', 0),
           # x one float off 16-byte alignment: the scalar-load kernels; big160 puts the one-lane epilogue on the f32 128 tile
           ('small', 'rows_f32_64_nt_slow', 'f32', 1), ('big160', 'rows_f32_128_nt_slow', 'f32', 1)]


@pytest.mark.parametrize('name,variant,kernel,mis', FWD_F32)
def test_fused_forward_fp32(H, name, variant, kernel, mis):
    check_fwd(H, name, variant, kernel, mis)


@pytest.mark.parametrize('name,variant', [('small', 'rows_b3_64'), ('big160', 'rows_b3p')])
def test_fused_forward_bf16_mode(H, name, variant):
    """bf16 operands, fp32 accumulation: x12 against the product of the bf16-rounded operands; small is the LDS form on
    the b3 kernel.  The gate reads fp32 x and is held to the same gate bound."""
    got12, _ = check_fwd(H, name, variant, 'bf16')
    exact = fwd_ref(name, False, False)[4]
    err = float(np.abs(got12 - exact).max() / np.abs(exact).max())
    assert 1e-4 < err < 3e-2, err                                     # genuinely bf16 operands, not fp32


@pytest.mark.parametrize('name,variant,kernel', [('small', 'rows_f32_64_nt_fast', 'f32'), ('big160', 'rows_b3p', 'b3')])
def test_fused_forward_special_values(H, name, variant, kernel):
    """saturated gates on every row, the last one and the ragged last tile included (y2 near +-30, +-90, +-200: sigmoid
    rounds to 1, expf overflows to +inf and underflows to 0) and units with y1 = +0 exactly (zero W1 row, b1 = +-0)"""
    got12, got = check_fwd(H, name, variant, kernel, special=True)
    rows, C = R.SHAPES[name]
    sat, zero = R.special_units(C)
    x = fwd_ref(name, True, False)[0]
    assert not got12[:, zero].any(), 'y1 of a unit with a zero W1 row and b1 = 0'
    assert np.array_equal(bits(got[:, sat[5]]), bits(x[:, sat[5]])), 'y2 = -200: the gate is shut, out = x'
    for u in (sat[0], sat[4]):                                        # y2 = +30, +200: the gate is open, out = relu(y1)
        assert np.array_equal(got[:, u], np.maximum(got12[:, u], 0))


# ---------------------------------------------------------------------------------------------------
# 5. the element-wise gate kernels
# ---------------------------------------------------------------------------------------------------
def gate_fwd_dev(H, x12_ptr, xd, rows, C):
    out = Out(rows, C, flat=True)
    counted(H, {}, lambda: _call('ft_highway_gate_fwd', x12_ptr, ptr(xd), out.ptr, rows, C, H._stream()))
    return out


@pytest.mark.parametrize('rows,C', R.GATE_SHAPES)
def test_gate_kernels(H, rows, C):
    dout, x12, x = R.gate_inputs(rows, C, 11)
    doutd, x12d, xd = op(dout), op(x12), op(x)
    want, _, bound = R.gate(x12, x)
    worst(fetch(gate_fwd_dev(H, ptr(x12d), xd, rows, C)), want, bound, f'gate_fwd {rows}x{C}')
    d12, dx = Out(rows, 2 * C, flat=True), Out(rows, C, flat=True)
    counted(H, {}, lambda: _call('ft_highway_gate_bwd', ptr(doutd), ptr(x12d), ptr(xd), d12.ptr, dx.ptr, rows, C,
                                 H._stream()))
    (wa, wb, wx), (ba, bb, bx) = R.gate_bwd(dout, x12, x)
    got12 = fetch(d12)
    worst(got12[:, :C], wa, ba, f'gate_bwd {rows}x{C} d12a')
    worst(got12[:, C:], wb, bb, f'gate_bwd {rows}x{C} d12b')
    worst(fetch(dx), wx, bx, f'gate_bwd {rows}x{C} dx')
    assert not got12[:, :C][x12[:, :C] == 0].any(), 'y1 = +-0: the ReLU derivative is 0'


@pytest.mark.parametrize('name,variant,special,same', [('tiny77', 'rows_f32_64_nt_fast', False, True),
                                                       ('small', 'rows_f32_64_nt_fast', True, True),
                                                       ('big160', 'rows_b3p', True, False)])
def test_gate_kernel_restates_the_fused_epilogue(H, name, variant, special, same):
    """ft_highway_gate_fwd on the x12 the fused forward stored against the fused forward's out: they state the same
    arithmetic.  The LDS form in ft_gemm_rows_kernel compiles to the kernel's very roundings: bit-equal.  The one-lane form
    in the pipelined kernel is contracted differently by the compiler (another choice of which product of
    g relu(y1) + (1 - g) x is fused into the sum): measured largest difference 4 u, one ulp of an |out| in [2, 4) -- there
    both are held to the gate bound of the float64 gate of the same x12."""
    rows, C = R.SHAPES[name]
    x, w12i, b1, b2, _, _ = fwd_ref(name, special, False)
    xd = op(x)
    out, x12 = fused_fwd(H, xd, op(w12i), op(b1), op(b2), rows, C, variant)
    got12, fused, alone = fetch(x12), fetch(out), fetch(gate_fwd_dev(H, x12.ptr, xd, rows, C))
    diff = float(np.abs(fused.astype(np.float64) - alone).max() / R.U)
    print(f'    gate_fwd vs fused {name}: largest difference = {diff:.3f} u')
    if same:
        assert np.array_equal(bits(fused), bits(alone))
    want, _, bound = R.gate(got12, x)
    worst(fused, want, bound, f'gate_fwd vs fused {name}, fused')
    worst(alone, want, bound, f'gate_fwd vs fused {name}, kernel')


# ---------------------------------------------------------------------------------------------------
# 6. / 7. ft_highway_bwd_data: dx += d12[:, :C] W1 + d12[:, C:] W2 (lda = 2C, contraction 2C, the prior as the bias),
# plain and with the gate gradient of the layer below in the epilogue (mode 2)
# ---------------------------------------------------------------------------------------------------
BWD = [('small', 1, 'rows_f32_64_nt_fast', 'f32'), ('big160', 1, 'rows_b3p', 'b3'), ('big96', 1, 'rows_b3p', 'b3'),
       ('small', 0, 'rows_f32_64_nn_fast', 'f32'), ('big160', 0, 'rows_f32_128_nn_fast', 'f32'),
       ('small', 1, 'rows_b3_64', 'bf16'), ('big160', 1, 'rows_b3p', 'bf16')]


@functools.lru_cache(maxsize=None)
def bwd_ref(name, bf16):
    rows, C = R.SHAPES[name]
    g = np.random.default_rng(SEEDS[name] + 50)
    d12 = wide(g, rows, 2 * C, 2.0)
    prior = wide(g, rows, C, 3.0)
    w1, w2 = (g.standard_normal((C, C)) / np.sqrt(C)).astype(f32), (g.standard_normal((C, C)) / np.sqrt(C)).astype(f32)
    dv, mag = R.data_grad(d12, w1, w2, prior, bf16)
    xb, bw1, bb1, bw2, bb2 = R.layer(rows, C, SEEDS[name] + 60, special=True)      # the layer below: planted values
    x12b = R.preact(xb, bw1, bb1, bw2, bb2)[0].astype(f32)
    return d12, prior, w1, w2, dv, mag, x12b, xb


def run_bwd_data(H, name, nt, variant, kernel, below):
    rows, C = R.SHAPES[name]
    d12, prior, w1, w2, dv, mag, x12b, xb = bwd_ref(name, kernel == 'bf16')
    d12d = op(d12, ld=2 * C)
    wad, wbd = (op(np.ascontiguousarray(w1.T)), op(np.ascontiguousarray(w2.T))) if nt else (op(w1), op(w2))
    dx = Out(rows, C, torch.from_numpy(prior), flat=True)
    x12bd, xbd, d12b = (op(x12b), op(xb), Out(rows, 2 * C, flat=True)) if below else (None, None, None)
    with bf16_mode(H, kernel == 'bf16'):
        counted(H, variant, lambda: _call('ft_highway_bwd_data', ptr(d12d), ptr(wad), ptr(wbd), nt, dx.ptr, rows, C,
                                          ptr(x12bd), ptr(xbd), d12b.ptr if below else None, H._stream()))
    return fetch(dx), fetch(d12b) if below else None, dv, R.gemm_bound(mag, prior, 2 * C, kernel), x12b, xb


@pytest.mark.parametrize('name,nt,variant,kernel', BWD)
def test_chained_data_gradient(H, name, nt, variant, kernel):
    got, _, dv, E, _, _ = run_bwd_data(H, name, nt, variant, kernel, below=False)
    worst(got, dv, E, f'bwd_data {name} {variant} {kernel} dx')


@pytest.mark.parametrize('name,nt,variant,kernel', BWD)
def test_chained_data_gradient_with_the_gate_below(H, name, nt, variant, kernel):
    C = R.SHAPES[name][1]
    got, got12, dv, E, x12b, xb = run_bwd_data(H, name, nt, variant, kernel, below=True)
    (wa, wb, wx), (ba, bb, bx) = R.bwd_data_below(dv, E, x12b, xb)
    tag = f'bwd_data below {name} {variant} {kernel}'
    worst(got12[:, :C], wa, ba, tag + ' d12a')
    worst(got12[:, C:], wb, bb, tag + ' d12b')
    worst(got, wx, bx, tag + ' dx')
    zero = x12b[:, :C] == 0
    assert zero.sum() == 3 * x12b.shape[0] and not got12[:, :C][zero].any(), 'y1 = +-0: the ReLU derivative is 0'


def test_data_gradient_refuses_half_a_layer_below(H):
    from forwardtacotron_amd._lib import FtError
    rows, C = 77, 32
    d12, w = op(np.ones((rows, 2 * C)), ld=2 * C), op(np.ones((C, C)))
    x12b, xb = op(np.ones((rows, 2 * C))), op(np.ones((rows, C)))
    for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        dx, d12b = Out(rows, C, flat=True), Out(rows, 2 * C, flat=True)
        with pytest.raises(FtError, match='go together'):
            _call('ft_highway_bwd_data', ptr(d12), ptr(w), ptr(w), 1, dx.ptr, rows, C, ptr(x12b) if mask[0] else None,
                  ptr(xb) if mask[1] else None, d12b.ptr if mask[2] else None, H._stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(dx.buf).all()) and bool(torch.isnan(d12b.buf).all()), 'refused, yet something was launched'


# ---------------------------------------------------------------------------------------------------
# 8. the stack as a composition
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,C,layers', [(300, 160, 3), (12300, 160, 2), (77, 9, 2)])
def test_stack_is_the_chain_of_kernel_calls(H, rows, C, layers, monkeypatch):
    """ops.highway_stack under autograd: y and dx bit-equal to the explicit chain of kernel calls (C = 9: the unfused
    HighwayFn, C % 32 != 0); every layer's dW1, dW2 (element-wise and by rel_err, the bars of test_tn_big_tile_tails) and
    db1, db2 (the bar of test_batched_column_sums_are_bit_identical_to_one_call_each) against float64 products of the
    chain's own d12_i and x_i -- which pins the `p + C * 4` offsets and the leading dimension 2C of the emitted gradients."""
    from forwardtacotron_amd import ops
    monkeypatch.delenv('FT_HIGHWAY_FUSED', raising=False)
    g = torch.Generator().manual_seed(rows + C)

    class Hw:                                    # parameter containers like model.HighwayNetwork
        def __init__(self):
            self.W1 = torch.nn.Linear(C, C)
            self.W2 = torch.nn.Linear(C, C)
            for p in (self.W1.weight, self.W2.weight):
                p.data = torch.randn(C, C, generator=g) * (1.0 / C ** 0.5)
            for p in (self.W1.bias, self.W2.bias):
                p.data = torch.randn(C, generator=g) * 0.3
            self.W1.cuda(); self.W2.cuda()

    hs = [Hw() for _ in range(layers)]
    P = [(h.W1.weight, h.W1.bias, h.W2.weight, h.W2.bias) for h in hs]
    x = torch.randn(rows, C, generator=g).cuda()
    wgt = torch.randn(rows, C, generator=g).cuda()
    xg = x.clone().requires_grad_(True)
    y = ops.highway_stack(xg, hs)
    (y * wgt).sum().backward()

    fused = C % 32 == 0
    with torch.no_grad():
        xs, x12s, d12s = [x], [], [None] * layers
        for w1, b1, w2, b2 in P:
            if fused:
                out, x12 = H.highway_fwd(xs[-1], H.highway_pack(w1, w2), b1, b2, save=True)
            else:
                x12 = H.linear_multi_fwd(xs[-1], [w1, w2], [b1, b2])
                out = H.highway_gate_fwd(x12, xs[-1])
            xs.append(out)
            x12s.append(x12)
        if fused:
            d12, dx = H.highway_gate_bwd(wgt, x12s[-1], xs[layers - 1])
            for i in range(layers - 1, -1, -1):
                d12s[i] = d12
                d12 = H.highway_bwd_data(d12, P[i][0], P[i][2], dx, below=(x12s[i - 1], xs[i - 1]) if i > 0 else None)
        else:
            dx = wgt
            for i in range(layers - 1, -1, -1):
                d12s[i], dx = H.highway_gate_bwd(dx, x12s[i], xs[i])
                p = d12s[i].data_ptr()
                H.linear_bwd_data_multi([p, p + C * 4], 2 * C, [P[i][0], P[i][2]], dx, rows, C, accumulate=True)
    assert torch.equal(y.detach(), xs[-1]) and bool(torch.isfinite(y).all())
    assert torch.equal(xg.grad, dx) and bool(torch.isfinite(dx).all())

    for i in range(layers):
        d, xi = d12s[i].double().cpu(), xs[i].double().cpu()
        for j, (half, what) in enumerate(((d[:, :C], 'W1'), (d[:, C:], 'W2'))):
            dw, db = P[i][2 * j].grad.cpu().double(), P[i][2 * j + 1].grad.cpu().double()
            ref, scale = half.t() @ xi, half.abs().t() @ xi.abs()
            e_elem, e_rel = float(((dw - ref).abs() / (scale + 1e-30)).max()), rel_err(dw, ref)
            e_bias = float((db - half.sum(0)).abs().max() / max(1.0, float(half.abs().sum(0).max())))
            print(f'    stack {rows}x{C} layer {i} {what}: dW element-wise {e_elem:.2e} (bar 1e-6), rel_err {e_rel:.2e} '
                  f'(bar 2e-6); db {e_bias:.2e} (bar 1e-5)')
            assert e_elem < 1e-6 and e_rel < 2e-6, (i, what)
            assert e_bias <= 1e-5, (i, what)
