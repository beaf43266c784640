"""CPU restatement, in float64 numpy, of the HighwayNetwork kernels (common_layers.py:35-40) and the a-priori rounding
bounds tests/test_gpu_highway.py holds them to:

  pack            the 32-row interleave of W1 / W2 (ft_highway_pack_kernel), the B operand of the fused forward
  preact          y1 | y2 = x W1^T + b1 | x W2^T + b2 and the magnitude sum|x||w| + |b| the GEMM bounds scale with
  gate            out = g relu(y1) + (1 - g) x, g = sigmoid(y2)      (ft_highway_epilogue mode 1, ft_highway_fwd_kernel)
  gate_bwd        d12 = dout g [y1 > 0] | dout (relu(y1) - x) g (1 - g), dx = dout (1 - g)     (ft_highway_bwd_kernel)
  bwd_data_below  the same three from a GEMM result dv known to +-E             (ft_highway_epilogue mode 2)

Every kernel is tested FROM ITS OWN fp32 INPUTS: the gate functions take the stored fp32 pre-activations x12, so the
reference never re-makes a ReLU decision and every element can be held to a bound.  u = 2^-24 (lens_cpu.U) is one fp32
rounding; the GEMM bounds are lens_cpu.conv_f32_bound / conv_b3_bound with k = 1.  tests/test_highway_cpu.py proves the
functions against float64 autograd, shows that an all-float32 evaluation stays inside the bounds without sitting far
below them, and asserts what the fixtures at the end of this file claim to contain.  No GPU, no project kernel.
Test-side only."""
import numpy as np

from lens_cpu import U, bf16_round, conv_b3_bound, conv_f32_bound, f64

TINY = 2.0 ** -126                  # smallest normal fp32
FLOOR = 4 * TINY                    # absolute floor of every gate bound: a product that lands below the normal range


# ---- pack ------------------------------------------------------------------------------------------------------------
def pack(w1, w2):
    """W1, W2 [C, C] (C % 32 == 0) -> [2C, C]: row n is row (n // 64) * 32 + n % 32 of W1 if n % 64 < 32, else of W2 --
    so output columns 64 j .. 64 j + 31 of the product are y1 of units 32 j .. 32 j + 31 and the next 32 their y2"""
    w1, w2 = np.asarray(w1), np.asarray(w2)
    C = w1.shape[0]
    assert C % 32 == 0 and w1.shape == w2.shape == (C, C)
    n = np.arange(2 * C)
    unit = (n // 64) * 32 + n % 32
    return np.where((n % 64 < 32)[:, None], w1[unit], w2[unit])


# ---- the products ----------------------------------------------------------------------------------------------------
def preact(x, w1, b1, w2, b2, bf16=False):
    """-> (y [rows, 2C] float64 = y1 | y2, mag = sum|x||w| + |b| per element).  bf16: x and the weights are rounded to the
    nearest bf16 first (the bf16 precision mode: products of bf16 operands are exact in fp32), the biases are not."""
    if bf16:
        x, w1, w2 = (bf16_round(f64(t).astype(np.float32)) for t in (x, w1, w2))
    x, w, b = f64(x), np.concatenate([f64(w1), f64(w2)]), np.concatenate([f64(b1), f64(b2)])
    return x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)


def data_grad(d12, w1, w2, prior, bf16=False):
    """-> (dv [rows, C] float64 = d12[:, :C] W1 + d12[:, C:] W2 + prior, mag = the same over absolute values): the chained
    data gradient, contraction length 2C, the prior content of dx in the part of the bias.  bf16: d12 and the weights
    rounded to bf16 first, the prior not."""
    if bf16:
        d12, w1, w2 = (bf16_round(f64(t).astype(np.float32)) for t in (d12, w1, w2))
    d, w, p = f64(d12), np.concatenate([f64(w1), f64(w2)]), f64(prior)
    return d @ w + p, np.abs(d) @ np.abs(w) + np.abs(p)


def gemm_bound(mag, bias, K, kernel):
    """kernel: 'f32' (ft_gemm_rows_kernel: exact products, K + 2 roundings), 'b3' (the bf16-split kernels in fp32 mode)
    or 'bf16' (the same kernels on one bf16 plane) -- lens_cpu's bounds for a 1-tap convolution over K channels"""
    if kernel == 'f32':
        return conv_f32_bound(mag, K, 1)
    return conv_b3_bound(mag, bias, K, 1, kernel == 'bf16')


# ---- the gate --------------------------------------------------------------------------------------------------------
def _sigmoid(y2):
    e = np.exp(-np.abs(y2))                              # no overflow in the reference
    return np.where(y2 >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _gate_terms(x12):
    """y1, relu(y1), g, 1 - g (float64; 1 - g formed without cancellation), and the absolute error bounds of the device's
    g and 1 - g.

    The kernels form g = 1.0f / (1.0f + expf(-y2)).  The device library's expf is accurate to 1 ulp (ROCm's OCML
    documentation lists exp at 1 ulp for fp32, the OpenCL full-profile figure), i.e. e = exp(-y2)(1 + 2u) at worst; 1 + e
    and the division (correctly rounded: the build does not relax fp32 division) take one rounding each.  The error of e
    reaches g through e / (1 + e) = 1 - g <= 1, so g carries at most (2u (1 - g) + 2u) g <= 4u g.  1 - g then carries that
    absolute error plus its own rounding u (1 - g).
    Below the normal range the relative statement ends: once 1 + e overflows or 1 / (1 + e) is a subnormal that the
    hardware may flush, g is wrong by up to 2^-126 absolutely (g_sub), whatever it is multiplied with afterwards."""
    x12 = f64(x12)
    C = x12.shape[-1] // 2
    y1, y2 = x12[..., :C], x12[..., C:]
    g = _sigmoid(y2)
    omg = _sigmoid(-y2)
    return y1, np.maximum(y1, 0.0), g, omg, 4 * U * g, 4 * U * g + U * omg


def gate(x12, x):
    """x12 [rows, 2C] = y1 | y2 (the fp32 values the device stored), x [rows, C] -> (out, g, bound), float64.

      out = fl(fl(g r) + fl(fl(1 - g) x)),  r = relu(y1)  (exact)

      fl(g r)           error <= (4u g + u g) r                     g's error, one rounding
      fl(fl(1 - g) x)   error <= (4u g + u (1 - g) + u (1 - g)) |x|   the error of 1 - g, one rounding
      the sum           error <= u |out|

      |err| <= (4u g + u g) r + (4u g + 2u (1 - g)) |x| + u |out| + floor,   floor = 2^-126 (4 + r + |x|)

    The floor is absolute: 4 * 2^-126 for products and sums that land below the normal range (kept or flushed
    subnormals must not decide a case) and 2^-126 (r + |x|) for g_sub of _gate_terms, which both terms multiply.  Terms of
    order u^2 are dropped.  A fused multiply-add only removes roundings."""
    y1, r, g, omg, eg, eomg = _gate_terms(x12)
    x = f64(x)
    out = g * r + omg * x
    bound = (eg + U * g) * r + (eomg + U * omg) * np.abs(x) + U * np.abs(out) + FLOOR + TINY * (r + np.abs(x))
    return out, g, bound


def _gate_bwd_coeffs(x12, x):
    """The three outputs are linear in dout: output = dout * c.  -> (ca, cb, cx) and (ka, kb, kx) with
    |device - dout c| <= |dout| k + floor:

      d12a = fl(dout g) [y1 > 0]                         ka = 4u g + u |ca|
      dx   = fl(dout fl(1 - g))                          kx = 4u g + u (1 - g) + u |cx|
      d12b = fl(fl(fl(dout fl(r - x)) g) fl(1 - g))      kb = 8u |cb| + |(r - x) g| (4u g + u (1 - g))
             (r - x, three products: 4 roundings; g's relative error 4u; then the absolute error of 1 - g)

    g_sub of _gate_terms adds 2^-126 to ka and kx and 2^-125 |r - x| to kb (once through g, once through 1 - g).
    y1 > 0 is strict: y1 = +-0 gives d12a = 0 exactly (k = 0 there, only the floor remains)."""
    y1, r, g, omg, eg, eomg = _gate_terms(x12)
    x = f64(x)
    pos = y1 > 0
    ca = np.where(pos, g, 0.0)
    cb = (r - x) * g * omg
    cx = omg
    ka = np.where(pos, eg + U * g + TINY, 0.0)
    kb = 8 * U * np.abs(cb) + np.abs((r - x) * g) * eomg + 2 * TINY * np.abs(r - x)
    kx = eomg + U * omg + TINY
    return (ca, cb, cx), (ka, kb, kx)


def gate_bwd(dout, x12, x):
    """-> ((d12a, d12b, dx), (bound_a, bound_b, bound_x)), float64 [rows, C] each; the derivations stand in
    _gate_bwd_coeffs, each bound + the floor 4 * 2^-126"""
    d = f64(dout)
    c, k = _gate_bwd_coeffs(x12, x)
    return tuple(d * ci for ci in c), tuple(np.abs(d) * ki + FLOOR for ki in k)


def bwd_data_below(dv, E, x12_below, x_below):
    """The mode-2 epilogue: the GEMM leaves dv' = dv + e, |e| <= E (dv = the float64 product + prior, E its GEMM bound),
    and applies the gate gradient of the layer below to dv'.  Each output is linear in dv, so
    |device - dv c| <= |c| E + (|dv| + E) k + floor: the GEMM error carried through the coefficient, plus the gate_bwd
    bound at the value the device held."""
    dv, E = f64(dv), f64(E)
    c, k = _gate_bwd_coeffs(x12_below, x_below)
    return tuple(dv * ci for ci in c), tuple(np.abs(ci) * E + (np.abs(dv) + E) * ki + FLOOR for ci, ki in zip(c, k))


# ---- an all-float32 evaluation (numpy), for test_highway_cpu.py's bound sanity check -------------------------------------
def gate_f32(x12, x):
    f = np.float32
    x12, x = np.asarray(x12, dtype=f), np.asarray(x, dtype=f)
    C = x12.shape[-1] // 2
    y1, y2 = x12[..., :C], x12[..., C:]
    with np.errstate(over='ignore', under='ignore'):
        g = f(1) / (f(1) + np.exp(-y2))
        return g * np.maximum(y1, f(0)) + (f(1) - g) * x, g


def gate_bwd_f32(dout, x12, x):
    f = np.float32
    dout, x12, x = (np.asarray(t, dtype=f) for t in (dout, x12, x))
    C = x12.shape[-1] // 2
    y1, y2 = x12[..., :C], x12[..., C:]
    with np.errstate(over='ignore', under='ignore'):
        g = f(1) / (f(1) + np.exp(-y2))
        d12a = np.where(y1 > 0, dout * g, f(0))
        d12b = dout * (np.maximum(y1, f(0)) - x) * g * (f(1) - g)
        return d12a, d12b, dout * (f(1) - g)


# ---- fixtures of tests/test_gpu_highway.py ---------------------------------------------------------------------------
# rows x C of the fused kernels: the smallest that reach each form (gemm_plan::tiles_big: >= 192 tiles of 128 x 128, N > 64)
SHAPES = {
    'tiny1': (1, 32), 'tiny77': (77, 32),   # N = 64: one 64-column tile, the LDS gate form
    'edge64': (65, 96),                     # one row past a 64-row tile; C % 64 = 32
    'small': (300, 160),                    # 64-tile; ragged rows and columns
    'big160': (12300, 160),                 # forward 97 x 3 tiles of 128, backward 97 x 2; rows % 128 = 12; the third column
                                            # tile holds units 128..159 in wave 0 and nothing in wave 1
    'big96': (24700, 96),                   # forward 193 x 2, backward 193 x 1; rows % 128 = 124; 2nd column tile half masked
}
GATE_SHAPES = [(77, 9), (300, 40), (24700, 96)]          # the element-wise kernels: the last crosses many 256-thread blocks
SAT = (30.0, -30.0, 90.0, -90.0, 200.0, -200.0)


def special_units(C):
    """-> (units whose b2 is SAT[i], units whose W1 row and b1 are zero; the last of those has b1 = -0.0)"""
    sat = [1, C // 4 + 1, C // 2 + 3, C // 2 + 7, C - 30, C - 1]
    zero = [0, C // 2 + 9, C - 2]
    assert len(set(sat + zero)) == 9 and all(0 <= u < C for u in sat + zero)
    return sat, zero


def layer(rows, C, seed, special=False):
    """fp32 operands of one highway layer: x [rows, C] ~ N(0, 1), W ~ N(0, 1 / C), b ~ 0.3 N(0, 1).  special: the planted
    units of special_units -- saturated gates on every row (y2 = b2 + N(0, 1): sigmoid rounds to 1 at +30, expf overflows
    to +inf around -90 and at -200, underflows to 0 at +200) and pre-activations y1 = +0 exactly."""
    g = np.random.default_rng(seed)
    f = np.float32
    x = g.standard_normal((rows, C)).astype(f)
    w1, w2 = (g.standard_normal((C, C)) / np.sqrt(C)).astype(f), (g.standard_normal((C, C)) / np.sqrt(C)).astype(f)
    b1, b2 = (0.3 * g.standard_normal(C)).astype(f), (0.3 * g.standard_normal(C)).astype(f)
    if special:
        sat, zero = special_units(C)
        b2[sat] = SAT
        w1[zero] = 0
        b1[zero] = 0
        b1[zero[-1]] = -0.0
    return x, w1, b1, w2, b2


def plant(x12, seed):
    """x12 [rows, 2C] fp32 (random) with the special values written in, in place: in the last row and in 40 random rows,
    y2 = SAT on the first six units and y1 = +0 / -0 on the last two (C >= 8)"""
    rows, C = x12.shape[0], x12.shape[1] // 2
    g = np.random.default_rng(seed)
    rs = np.unique(np.concatenate([[rows - 1], g.integers(0, rows, 40)]))
    for i, v in enumerate(SAT):
        x12[rs, C + i] = v
    x12[rs, C - 2] = 0.0
    x12[rs, C - 1] = -0.0
    return x12


def gate_inputs(rows, C, seed):
    """(dout, x12, x) fp32 for the element-wise kernels: random, planted"""
    g = np.random.default_rng(seed)
    f = np.float32
    x12 = plant((2 * g.standard_normal((rows, 2 * C))).astype(f), seed + 1)
    return g.standard_normal((rows, C)).astype(f), x12, g.standard_normal((rows, C)).astype(f)
