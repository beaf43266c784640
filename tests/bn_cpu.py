"""CPU restatement, in float64 numpy, of the BatchNorm family behind forwardtacotron_amd/csrc/ft_bn.hip and of the
statistics the 128x128 split GEMM leaves in its epilogue, written from torch.nn.BatchNorm1d's definition:

  training statistics  mean / BIASED variance over the B * tvalid(c) valid positions of channel c; running statistics
                       take the UNBIASED variance with the given momentum;
  CBHG bank buffer     y [B, Tbuf, K*group]: the BatchNorm of an odd-k member (channel group 0, 2, ..) sees Tbuf - 1
                       rows, that of an even-k member all Tbuf; the caller slices [:Tout] afterwards;
  pool                 MaxPool1d(2, 1, 1)[:T], i.e. out[t] = max(z[t-1], z[t]); a window's gradient goes to its FIRST
                       maximal element (z[t-1] on a tie).

Rows at t >= tvalid(c) are never read (they may hold NaN).  `eps` and `momentum` are fp32 arguments of the C ABI: they
are rounded to fp32 first, everything after that is float64.  tests/test_bn_cpu.py proves these functions against
torch's float64 batch_norm / max_pool1d / relu and autograd.  Test-side only."""
import numpy as np


def f64(t):
    """float64 numpy copy of a numpy array or a torch tensor (any device)"""
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def tvalid(c, Tbuf, group):
    """rows of channel c its BatchNorm sees: Tbuf - 1 for the members with an odd kernel width (group index even)"""
    return Tbuf - 1 if (group > 0 and ((c // group) + 1) % 2 == 1) else Tbuf


def tvalid_all(C, Tbuf, group):
    return np.array([tvalid(c, Tbuf, group) for c in range(C)], dtype=np.int64)


def valid_mask(Tbuf, C, group):
    """bool [Tbuf, C]: t < tvalid(c)"""
    return np.arange(Tbuf)[:, None] < tvalid_all(C, Tbuf, group)[None, :]


def poison(y, group, value=np.nan):
    """copy of y [B, Tbuf, C] with `value` at every position no kernel may read"""
    y = np.array(y, copy=True)
    B, Tbuf, C = y.shape
    y[:, ~valid_mask(Tbuf, C, group)] = value
    return y


def sums(y, group, r0=0, r1=None):
    """[C, 2]: (sum, sum of squares) of every channel over its valid rows among the flat rows r0 <= b * Tbuf + t < r1"""
    y = f64(y)
    B, Tbuf, C = y.shape
    r1 = B * Tbuf if r1 is None else min(r1, B * Tbuf)
    rows = np.arange(B * Tbuf)
    m = valid_mask(Tbuf, C, group)[rows % Tbuf] & ((rows >= r0) & (rows < r1))[:, None]
    v = np.where(m, y.reshape(B * Tbuf, C), 0.0)
    return np.stack([v.sum(0), (v * v).sum(0)], axis=1)


def abs_sums(y, group, r0=0, r1=None):
    """[C, 2]: (sum |y|, sum y^2) over the same rows: the magnitudes a summation-error bound scales with"""
    y = f64(y)
    B, Tbuf, C = y.shape
    return sums(np.where(valid_mask(Tbuf, C, group)[None], np.abs(y), 0.0), group, r0, r1)


def chunk_partials(y, group, rows_per_chunk, nchunks):
    """[nchunks, C, 2]: sums() of every run of rows_per_chunk flat rows (the last run may be short)"""
    y = f64(y)
    B, Tbuf, C = y.shape
    pad = nchunks * rows_per_chunk - B * Tbuf
    assert pad >= 0, (B * Tbuf, rows_per_chunk, nchunks)
    v = np.where(valid_mask(Tbuf, C, group)[None], y, 0.0).reshape(B * Tbuf, C)
    v = np.concatenate([v, np.zeros((pad, C))]).reshape(nchunks, rows_per_chunk, C)
    return np.stack([v.sum(1), (v * v).sum(1)], axis=2)


def finalize(partials, B, Tbuf, group, momentum, eps, running_mean=None, running_var=None):
    """partials [nchunks, C, 2] -> (mean, rstd, new running_mean, new running_var); the variance is clamped at 0"""
    p = f64(partials).sum(0)
    C = p.shape[0]
    n = B * tvalid_all(C, Tbuf, group).astype(np.float64)
    eps = float(np.float32(eps))
    momentum = float(np.float32(momentum))
    mean = p[:, 0] / n
    var = np.maximum(p[:, 1] / n - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    if running_mean is None:
        return mean, rstd, None, None
    unbiased = np.where(n > 1, var * n / np.maximum(n - 1, 1), var)
    return (mean, rstd, (1 - momentum) * f64(running_mean) + momentum * mean,
            (1 - momentum) * f64(running_var) + momentum * unbiased)


def stats(y, group, eps):
    """(mean, biased variance, rstd) of every channel by the two-pass formula (no cancellation): the reference for
    finalize()'s one-pass E[y^2] - mean^2"""
    y = f64(y)
    B, Tbuf, C = y.shape
    m = valid_mask(Tbuf, C, group)[None]
    n = B * tvalid_all(C, Tbuf, group).astype(np.float64)
    mean = np.where(m, y, 0.0).sum((0, 1)) / n
    var = np.where(m, (y - mean) ** 2, 0.0).sum((0, 1)) / n
    return mean, var, 1.0 / np.sqrt(var + float(np.float32(eps)))


def xhat(y, mean, rstd):
    return (f64(y) - f64(mean)) * f64(rstd)


def apply(y, mean, rstd, gamma, beta, residual, Tout):
    """out [B, Tout, C] = (y - mean) * rstd * gamma + beta (+ residual)"""
    out = xhat(f64(y)[:, :Tout], mean, rstd) * f64(gamma) + f64(beta)
    return out if residual is None else out + f64(residual)


def pool(z):
    """out[t] = max(z[t-1], z[t]), out[0] = z[0]: MaxPool1d(kernel 2, stride 1, padding 1)[:T] over axis 1"""
    z = f64(z)
    out = z.copy()
    out[:, 1:] = np.maximum(z[:, :-1], z[:, 1:])
    return out


def pool_grad(dout, z):
    """dz of pool(): window t = (z[t-1], z[t]) sends dout[t] to z[t] only if z[t] > z[t-1] (first maximum wins)"""
    dout, z = f64(dout), f64(z)
    own = np.ones(z.shape, dtype=bool)
    own[:, 1:] = z[:, 1:] > z[:, :-1]
    dz = np.where(own, dout, 0.0)
    dz[:, :-1] += np.where(own[:, 1:], 0.0, dout[:, 1:])
    return dz


def bwd(dout, y, gamma, mean, rstd, group, relu):
    """backward of apply() through the statistics: dout [B, Tout, C] (zero beyond Tout) ->
    (dy [B, Tbuf, C], dgamma, dbeta); dy is 0 at t >= tvalid(c) and, with relu, where y <= 0 (y = relu(a): dy is da)"""
    dout, y = f64(dout), f64(y)
    B, Tbuf, C = y.shape
    Tout = dout.shape[1]
    m = valid_mask(Tbuf, C, group)[None]
    g = np.zeros((B, Tbuf, C))
    g[:, :Tout] = dout
    g = np.where(m, g, 0.0)
    xh = np.where(m, xhat(np.where(m, y, 0.0), mean, rstd), 0.0)
    n = B * tvalid_all(C, Tbuf, group).astype(np.float64)
    dbeta = g.sum((0, 1))
    dgamma = (g * xh).sum((0, 1))
    dy = bwd_apply(g, y, gamma, mean, rstd, dgamma, dbeta, group, relu)
    return dy, dgamma, dbeta


def bwd_apply(g, y, gamma, mean, rstd, dgamma, dbeta, group, relu):
    """dy = gamma * rstd * (g - dbeta / n - xhat * dgamma / n) from GIVEN column sums; g [B, Tbuf, C] already padded"""
    g, y = f64(g), f64(y)
    B, Tbuf, C = y.shape
    m = valid_mask(Tbuf, C, group)[None]
    ys = np.where(m, y, 0.0)
    n = B * tvalid_all(C, Tbuf, group).astype(np.float64)
    dy = f64(gamma) * f64(rstd) * (np.where(m, g, 0.0) - f64(dbeta) / n - xhat(ys, mean, rstd) * f64(dgamma) / n)
    if relu:
        dy = np.where(ys > 0, dy, 0.0)
    return np.where(m, dy, 0.0)


def pool_dz(dout, y, gamma, beta, mean, rstd):
    """gradient of the BatchNorm output under pool(): [B, Tout, C]"""
    Tout = f64(dout).shape[1]
    return pool_grad(dout, apply(y, mean, rstd, gamma, beta, None, Tout))


def pool_bwd(dout, y, gamma, beta, mean, rstd, group, relu):
    """backward of pool(apply(y)[:, :Tout]): dout is the gradient of the POOLED output"""
    return bwd(pool_dz(dout, y, gamma, beta, mean, rstd), y, gamma, mean, rstd, group, relu)


def fold_eval(gamma, beta, running_mean, running_var, eps):
    """eval-mode BatchNorm as one multiply-add: (scale, shift)"""
    scale = f64(gamma) / np.sqrt(f64(running_var) + float(np.float32(eps)))
    return scale, f64(beta) - f64(running_mean) * scale


# ---------------------------------------------------------------------------------------------------
# inputs shared by tests/test_bn_cpu.py and tests/test_gpu_batchnorm.py
# ---------------------------------------------------------------------------------------------------
EPS = 1e-5

# (B, Tbuf, C, group): every kernel path of ft_bn.hip -- 16-byte lanes (C and group multiples of 4) and the scalar
# kernels (C = 6, 70; group = 6, 35, 2), one chunk and several, row counts that are no multiple of 4 / 16 / 64
BN_CASES = ((5, 13, 64, 0), (3, 37, 64, 16), (7, 11, 6, 0), (2, 9, 6, 2), (3, 70, 70, 35), (9, 29, 70, 0),
            (2, 33, 12, 6), (1, 1, 64, 0), (1, 1, 6, 0),
            # C = 64 with 210 / 413 / 549 / 4347 rows: 4, 7, 9 and 64 chunks of the stand-alone reduction
            (3, 70, 64, 0), (7, 59, 64, 0), (9, 61, 64, 16), (27, 161, 64, 0))
BN_CHUNKS = {(5, 13, 64, 0): 2, (1, 1, 64, 0): 1, (3, 70, 64, 0): 4, (7, 59, 64, 0): 7, (9, 61, 64, 16): 9,
             (27, 161, 64, 0): 64, (3, 70, 70, 35): 4}

# (B, Tbuf, Tout, C, group) for the fused BatchNorm + MaxPool pair (16-byte lanes only)
POOL_CASES = ((3, 14, 13, 16, 4), (2, 2, 1, 8, 4), (2, 3, 2, 8, 4), (5, 41, 40, 64, 16), (4, 9, 9, 12, 0))


def bn_inputs(B, Tbuf, C, group, seed, poisoned=True):
    """fp32 a [B, Tbuf, C] (pre-activation, NaN where no kernel may read), gamma, beta, running stats; channel 0 is
    constant, channel 1 has mean 100 and standard deviation 1"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((B, Tbuf, C)).astype(np.float32)
    a[..., 0] = 0.75
    if C > 1:
        a[..., 1] += 100.0
    if poisoned:
        a = poison(a, group)
    gamma = rng.standard_normal(C).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    rm = rng.standard_normal(C).astype(np.float32)
    rv = (0.5 + rng.random(C)).astype(np.float32)
    return a, gamma, beta, rm, rv


def pool_inputs(B, Tbuf, Tout, C, group, seed):
    """y [B, Tbuf, C]: multiples of 1/8 in [0, 4], about a third exact zeros and many equal neighbours; |gamma| in
    [0.25, 1.25) with both signs; dout: multiples of 1/16 (the sum of two of them is exact in fp32).  The pooling
    decisions z[t] > z[t-1] then cannot differ between fp32 and float64: equal y give bit-equal z, different y give z
    more than 1e-3 apart (asserted by tests/test_bn_cpu.py with pool_min_gap)."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 33, (B, Tbuf, C)).astype(np.float32) / 8
    y[rng.random((B, Tbuf, C)) < 0.33] = 0.0
    rep = rng.random((B, Tbuf, C)) < 0.3                      # runs of equal neighbours that are not zeros
    y[:, 1:][rep[:, 1:]] = y[:, :-1][rep[:, 1:]]
    y = poison(y, group)
    gamma = ((0.25 + rng.random(C)) * np.where(rng.random(C) < 0.5, -1.0, 1.0)).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    dout = (rng.integers(-32, 33, (B, Tout, C)) / 16).astype(np.float32)
    return y, gamma, beta, dout


def pool_min_gap(z):
    """(smallest non-zero |z[t] - z[t-1]|, number of exact ties) along axis 1"""
    d = np.abs(np.diff(f64(z), axis=1))
    nz = d[d > 0]
    return (float(nz.min()) if nz.size else np.inf), int((d == 0).sum())
