"""CPU: tests/highway_cpu.py itself.  gate / gate_bwd chained over three layers equal float64 autograd through the
oracle's HighwayNetwork; pack equals its definition written as a loop; an evaluation of the gate in numpy float32 stays
inside the a-priori bounds and does not sit absurdly far below them (each worst ratio is printed: pytest -s); and the
fixtures the GPU tests use contain what they claim."""
import numpy as np
import pytest
import torch

import highway_cpu as R
from oracle import ft_oracle as O


def test_gate_chain_equals_float64_autograd():
    rows, C, L = 37, 12, 3
    g = torch.Generator().manual_seed(2)
    P = {}
    for i in range(L):
        for n in ('W1', 'W2'):
            P[f'h{i}.{n}.weight'] = (torch.randn(C, C, generator=g, dtype=torch.float64) / C ** 0.5).requires_grad_(True)
            P[f'h{i}.{n}.bias'] = (0.3 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    x0 = torch.randn(rows, C, generator=g, dtype=torch.float64, requires_grad=True)
    wgt = torch.randn(rows, C, generator=g, dtype=torch.float64)
    y = x0
    for i in range(L):
        y = O.highway(y, P, f'h{i}.')
    (y * wgt).sum().backward()

    xs, x12s = [x0.detach().numpy()], []
    for i in range(L):
        x12, _ = R.preact(xs[-1], *(P[f'h{i}.{n}'].detach() for n in ('W1.weight', 'W1.bias', 'W2.weight', 'W2.bias')))
        assert np.abs(x12[:, :C]).min() > 1e-9, 'a ReLU pre-activation at rounding distance of 0: pick another seed'
        x12s.append(x12)
        xs.append(R.gate(x12, xs[-1])[0])
    assert np.abs(xs[-1] - y.detach().numpy()).max() <= 1e-13
    dout = wgt.numpy()
    for i in range(L - 1, -1, -1):
        (da, db, dx), _ = R.gate_bwd(dout, x12s[i], xs[i])
        w1, w2 = P[f'h{i}.W1.weight'], P[f'h{i}.W2.weight']
        for got, p in ((da.T @ xs[i], w1), (db.T @ xs[i], w2), (da.sum(0), P[f'h{i}.W1.bias']),
                       (db.sum(0), P[f'h{i}.W2.bias'])):
            assert np.abs(got - p.grad.numpy()).max() <= 1e-12
        dv, _ = R.data_grad(np.concatenate([da, db], 1), w1.detach(), w2.detach(), dx)
        if i > 0:                                     # bwd_data_below = gate_bwd of the chained product
            (ba, bb, bx), _ = R.bwd_data_below(dv, np.zeros_like(dv), x12s[i - 1], xs[i - 1])
            (ga, gb, gx), _ = R.gate_bwd(dv, x12s[i - 1], xs[i - 1])
            assert np.array_equal(ba, ga) and np.array_equal(bb, gb) and np.array_equal(bx, gx)
        dout = dv
    assert np.abs(dout - x0.grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize('C', [32, 96, 160])
def test_pack_equals_its_definition(C):
    g = np.random.default_rng(C)
    w1, w2 = g.standard_normal((C, C)).astype(np.float32), g.standard_normal((C, C)).astype(np.float32)
    want = np.empty((2 * C, C), dtype=np.float32)
    for n in range(2 * C):
        src = w1 if n % 64 < 32 else w2
        want[n] = src[(n // 64) * 32 + n % 32]
    got = R.pack(w1, w2)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # every row of W1 and of W2 appears exactly once
    assert sorted(map(bytes, got)) == sorted(map(bytes, np.concatenate([w1, w2])))


def test_float32_gate_holds_the_bounds_and_is_not_far_below_them():
    n = 2_000_000
    g = np.random.default_rng(0)
    f = np.float32
    y1 = (2 * g.standard_normal(n)).astype(f)
    y2 = np.where(np.arange(n) % 2 == 0, 3 * g.standard_normal(n), np.linspace(-120, 120, n)).astype(f)
    x = (2 * g.standard_normal(n)).astype(f)
    dout = g.standard_normal(n).astype(f)
    y1[::1000] = 0.0
    y1[1::1000] = -0.0
    x12 = np.stack([y1, y2], 1)
    x, dout = x[:, None], dout[:, None]
    out, _ = R.gate_f32(x12, x)
    want, _, bound = R.gate(x12, x)
    worst = {'out': float((np.abs(out - want) / bound).max())}
    got = R.gate_bwd_f32(dout, x12, x)
    wants, bounds = R.gate_bwd(dout, x12, x)
    for name, a, w, b in zip(('d12a', 'd12b', 'dx'), got, wants, bounds):
        assert np.all(np.isfinite(a))
        worst[name] = float((np.abs(a - w) / b).max())
    assert not got[0][::1000].any() and not got[0][1::1000].any(), 'y1 = +-0: the derivative is 0'
    for name, r in worst.items():
        print(f'    fp32 emulation, {name}: worst |err| / bound = {r:.3f}')
        assert 0.05 < r <= 1.0, (name, r)


def test_gemm_bound_is_lens_cpus():
    import lens_cpu as Lc
    mag = np.array([[3.0, 5.0]])
    bias = np.array([1.0, -2.0])
    assert np.array_equal(R.gemm_bound(mag, bias, 160, 'f32'), Lc.conv_f32_bound(mag, 160, 1))
    assert np.array_equal(R.gemm_bound(mag, bias, 160, 'b3'), Lc.conv_b3_bound(mag, bias, 160, 1, False))
    assert np.array_equal(R.gemm_bound(mag, bias, 160, 'bf16'), Lc.conv_b3_bound(mag, bias, 160, 1, True))


@pytest.mark.parametrize('name', ['small', 'big160'])
def test_special_layers_contain_their_plants(name):
    rows, C = R.SHAPES[name]
    rows = min(rows, 600)                              # the plants sit on units: every row carries them
    x, w1, b1, w2, b2 = R.layer(rows, C, 7, special=True)
    sat, zero = R.special_units(C)
    y, _ = R.preact(x, w1, b1, w2, b2)
    assert int((y[:, :C] == 0).sum()) == 3 * rows and not y[:, zero].any()
    assert np.signbit(b1[zero[-1]]) and not np.signbit(b1[zero[0]])
    for u, v in zip(sat, R.SAT):
        assert np.abs(y[:, C + u] - v).max() < 8.0
    _, g = R.gate_f32(y.astype(np.float32), x)
    assert (g[:, sat[0]] == 1).all() and (g[:, sat[5]] == 0).all() and (g[:, sat[3]] == 0).any()
    assert np.all(np.isfinite(R.gate_f32(y.astype(np.float32), x)[0]))
    # the plain layer has none of it
    y, _ = R.preact(*R.layer(rows, C, 7))
    assert not (y[:, :C] == 0).any() and np.abs(y).max() < 20


@pytest.mark.parametrize('rows,C', R.GATE_SHAPES)
def test_gate_inputs_contain_their_plants(rows, C):
    dout, x12, x = R.gate_inputs(rows, C, 11)
    assert dout.shape == x.shape == (rows, C) and x12.shape == (rows, 2 * C)
    y1, y2 = x12[:, :C], x12[:, C:]
    assert y1[-1, C - 2] == 0 and not np.signbit(y1[-1, C - 2]) and y1[-1, C - 1] == 0 and np.signbit(y1[-1, C - 1])
    assert int((y1 == 0).sum()) == 2 * int((y2[:, 0] == R.SAT[0]).sum()) >= 4
    assert tuple(y2[-1, :6]) == R.SAT
    _, g = R.gate_f32(x12, x)
    assert (g == 0).sum() >= 3 and (g == 1).sum() >= 2
    (da, _, _), _ = R.gate_bwd(dout, x12, x)
    assert not da[y1 == 0].any()


def test_shapes_reach_the_forms_they_are_named_for():
    """gemm_plan::tiles_big restated: >= 192 tiles of 128 x 128, N > 64, M > 64 (forward N = 2C; the chained backward
    counts one task's tiles, N = C)"""
    def big(rows, N):
        return -(-rows // 128) * -(-N // 128) >= 192 and N > 64 and rows > 64
    for name, (rows, C) in R.SHAPES.items():
        assert big(rows, 2 * C) == big(rows, C) == name.startswith('big'), name
        assert C % 32 == 0 and rows % 64 != 0
    assert R.SHAPES['big160'][0] % 128 == 12 and R.SHAPES['big96'][0] % 128 == 124
    assert R.SHAPES['edge64'] == (65, 96) and R.SHAPES['big96'][1] % 64 == 32
