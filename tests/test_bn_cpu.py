"""tests/bn_cpu.py (the float64 restatement the GPU BatchNorm tests compare with) against torch in float64:
torch.nn.functional.batch_norm, relu, max_pool1d(2, 1, 1)[:T] and autograd, per bank member -- an odd-k member's
BatchNorm sees Tbuf - 1 rows, an even-k member's Tbuf -- on the shapes tests/test_gpu_batchnorm.py runs.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cpu as R

EPS32 = float(np.float32(R.EPS))


def close(a, b, what=''):
    a, b = R.f64(a), R.f64(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.all(np.isfinite(a)), what
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9, err_msg=what)


def members(C, group):
    """channel slices that share one BatchNorm's row count"""
    if group == 0:
        return [slice(0, C)]
    return [slice(c0, min(c0 + group, C)) for c0 in range(0, C, group)]


def test_tvalid_is_the_bank_rule():
    # member i of a bank has kernel width k = i + 1; an even k yields T + 1 = Tbuf outputs, an odd k only T
    for group in (1, 4, 6, 35):
        for c in range(0, 6 * group):
            k = c // group + 1
            assert R.tvalid(c, 10, group) == (10 if k % 2 == 0 else 9)
    assert R.tvalid(123, 10, 0) == 10
    m = R.valid_mask(5, 4, 2)
    assert m[:4].all() and not m[4, :2].any() and m[4, 2:].all()


@pytest.mark.parametrize('B,Tbuf,C,group', R.BN_CASES)
@pytest.mark.parametrize('relu', [False, True])
def test_forward_and_backward_equal_torch(B, Tbuf, C, group, relu):
    momentum = 0.37 if relu else 0.1
    a, gamma, beta, rm, rv = R.bn_inputs(B, Tbuf, C, group, seed=B * 1000 + Tbuf)
    Tout = Tbuf - 1 if group > 0 else (Tbuf if B % 2 else max(Tbuf - 2, 1))
    rng = np.random.default_rng(5)
    dout = rng.standard_normal((B, Tout, C))
    res = rng.standard_normal((B, Tout, C))
    y = np.maximum(a, 0) if relu else a                    # NaN rows stay NaN: nothing below may read them
    assert np.isnan(y).any() == (group > 0)

    nch = 3
    rpc = -(-B * Tbuf // nch)
    part = R.chunk_partials(y, group, rpc, nch)
    close(part.sum(0), R.sums(y, group), 'chunks add up to the whole')
    mean, rstd, nrm, nrv = R.finalize(part, B, Tbuf, group, momentum, R.EPS, rm, rv)
    mean2, var2, rstd2 = R.stats(y, group, R.EPS)
    close(mean, mean2, 'mean'); close(rstd, rstd2, 'one-pass against two-pass rstd')
    out = R.apply(y, mean, rstd, gamma, beta, res, Tout)
    dy, dgamma, dbeta = R.bwd(dout, y, gamma, mean, rstd, group, relu)
    assert np.all(dy[:, ~R.valid_mask(Tbuf, C, group)] == 0)

    if B * Tbuf == 1:                                     # torch refuses one value per channel; by hand
        close(mean, y[0, 0], 'n = 1 mean')
        close(rstd, np.full(C, 1 / np.sqrt(EPS32)), 'n = 1 rstd')
        close(nrv, (1 - float(np.float32(momentum))) * R.f64(rv), 'n = 1: unbiased = biased = 0')
        close(out, R.f64(beta) + res, 'n = 1 out')
        close(dy, np.zeros_like(dy), 'n = 1 dy'); close(dgamma, np.zeros(C)); close(dbeta, dout[0, 0])
        return
    for sl in members(C, group):
        tv = R.tvalid(sl.start, Tbuf, group)
        at = torch.from_numpy(R.f64(a[:, :tv, sl])).requires_grad_(True)
        gt = torch.from_numpy(R.f64(gamma[sl])).requires_grad_(True)
        bt = torch.from_numpy(R.f64(beta[sl])).requires_grad_(True)
        rmt, rvt = torch.from_numpy(R.f64(rm[sl])), torch.from_numpy(R.f64(rv[sl]))
        yt = torch.relu(at) if relu else at
        zt = F.batch_norm(yt.transpose(1, 2), rmt, rvt, gt, bt, training=True, momentum=float(np.float32(momentum)),
                          eps=EPS32).transpose(1, 2)
        ot = zt[:, :Tout] + torch.from_numpy(res[:, :, sl])
        (ot * torch.from_numpy(dout[:, :, sl])).sum().backward()
        close(out[:, :, sl], ot.detach(), 'out')
        close(nrm[sl], rmt, 'running_mean'); close(nrv[sl], rvt, 'running_var')
        close(dy[:, :tv, sl], at.grad, 'dy'); close(dgamma[sl], gt.grad, 'dgamma'); close(dbeta[sl], bt.grad, 'dbeta')
        if tv > Tout:                                      # the row sliced off still belongs to the statistics
            assert np.abs(at.grad[:, Tout:].numpy()).max() > 0 or C * B < 4


def test_special_channels():
    a, gamma, beta, rm, rv = R.bn_inputs(4, 50, 8, 0, seed=3)
    mean, rstd, _, _ = R.finalize(R.chunk_partials(a, 0, 64, 4), 4, 50, 0, 0.1, R.EPS, rm, rv)
    assert mean[0] == 0.75 and rstd[0] == 1 / np.sqrt(EPS32)          # constant channel: variance exactly 0
    assert abs(mean[1] - 100) < 0.5 and 0.7 < rstd[1] < 1.4           # mean 100, standard deviation 1
    # a negative one-pass variance (rounding of E[y^2] - mean^2) is clamped, not passed to sqrt
    p = np.array([[[3.0, 2.9]]])                                      # mean 1, E[y^2] = 0.9667
    assert R.finalize(p, 1, 3, 0, 0.1, R.EPS)[1][0] == 1 / np.sqrt(EPS32)


@pytest.mark.parametrize('B,Tbuf,Tout,C,group', R.POOL_CASES)
@pytest.mark.parametrize('relu', [False, True])
def test_pool_equals_torch_and_ties_are_safe(B, Tbuf, Tout, C, group, relu):
    y, gamma, beta, dout = R.pool_inputs(B, Tbuf, Tout, C, group, seed=Tbuf)
    part = R.chunk_partials(y, group, B * Tbuf, 1)
    mean, rstd, _, _ = R.finalize(part, B, Tbuf, group, 0.1, R.EPS)
    z = R.apply(y, mean, rstd, gamma, beta, None, Tout)
    out = R.pool(z)
    dy, dgamma, dbeta = R.pool_bwd(dout, y, gamma, beta, mean, rstd, group, relu)
    # the condition the GPU comparison rests on: no pooling decision is closer than 1e-3, ties are exact and frequent,
    # and zeros (the ReLU's) are among the inputs
    gap, ties = R.pool_min_gap(z)
    assert gap > 1e-3, gap
    if Tout > 1:
        assert ties >= B * (Tout - 1) * C // 8, ties
    yv = y[:, :Tout]
    assert np.all(yv * 8 == np.round(yv * 8)) and yv.min() >= 0 and yv.max() <= 4
    assert (yv == 0).mean() > 0.2 or yv.size < 200
    assert np.abs(gamma).min() >= 0.25 and (gamma > 0).any() and (gamma < 0).any()
    for sl in members(C, group):
        tv = R.tvalid(sl.start, Tbuf, group)
        ys = R.f64(y[:, :tv, sl])
        at = torch.from_numpy(np.where(ys > 0, ys, -1.0) if relu else ys).requires_grad_(True)
        gt = torch.from_numpy(R.f64(gamma[sl])).requires_grad_(True)
        bt = torch.from_numpy(R.f64(beta[sl])).requires_grad_(True)
        yt = torch.relu(at) if relu else at
        zt = F.batch_norm(yt.transpose(1, 2), None, None, gt, bt, training=True, eps=EPS32)[:, :, :Tout]
        pt = F.max_pool1d(zt, kernel_size=2, stride=1, padding=1)[:, :, :Tout].transpose(1, 2)
        (pt * torch.from_numpy(R.f64(dout[:, :, sl]))).sum().backward()
        close(out[:, :, sl], pt.detach(), 'pooled')
        close(dy[:, :tv, sl], at.grad, 'dy'); close(dgamma[sl], gt.grad, 'dgamma'); close(dbeta[sl], bt.grad, 'dbeta')


def test_pool_grad_first_maximum():
    z = np.array([[[1.0], [1.0], [0.5], [2.0], [2.0], [2.0]]])
    d = np.arange(1.0, 7.0).reshape(1, 6, 1)
    assert R.pool(z)[0, :, 0].tolist() == [1, 1, 1, 2, 2, 2]
    # windows: (-, z0) -> z0; (z0, z1) tie -> z0; (z1, z2) -> z1; (z2, z3) -> z3; (z3, z4) tie -> z3; (z4, z5) tie -> z4
    assert R.pool_grad(d, z)[0, :, 0].tolist() == [1 + 2, 3, 0, 4 + 5, 6, 0]
    zt = torch.from_numpy(z).transpose(1, 2).clone().requires_grad_(True)
    (F.max_pool1d(zt, 2, 1, 1)[:, :, :6] * torch.from_numpy(d).transpose(1, 2)).sum().backward()
    assert zt.grad[0, 0].tolist() == [3, 3, 0, 9, 6, 0]


def test_fold_eval_equals_eval_mode_batch_norm():
    _, gamma, beta, rm, rv = R.bn_inputs(2, 3, 70, 0, seed=1)
    scale, shift = R.fold_eval(gamma, beta, rm, rv, R.EPS)
    x = np.random.default_rng(0).standard_normal((4, 70, 9))
    ref = F.batch_norm(torch.from_numpy(x), torch.from_numpy(R.f64(rm)), torch.from_numpy(R.f64(rv)),
                       torch.from_numpy(R.f64(gamma)), torch.from_numpy(R.f64(beta)), training=False, eps=EPS32)
    close(x * scale[None, :, None] + shift[None, :, None], ref, 'folded eval')
