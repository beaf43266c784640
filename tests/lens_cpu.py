"""CPU restatement, in plain numpy, of the small length-aware ("lens") inference kernels every generate_batch rests on:

  conv_bias_lens      nn.Conv1d(padding = k // 2) with bias (+ ReLU) per item, 0 past the item's length
                      (hip.conv1d_bias_fwd_lens: the bias arm of the GEMM epilogues under FtGemmBatch.out_lens)
  add_layernorm_lens  LayerNorm(x + res) per row, 0 past the length          (ft_add_layernorm_fwd_lens_kernel)
  transpose_pad_lens  [B,T,C] -> [B,C,Tout], `pad` past the length           (ft_transpose_pad_lens_kernel)
  gen_durations       what generate() and the LengthRegulator do to the predicted durations of ONE item: the fallback
                      `dur.long().sum() <= 0 -> fill 2.`, the clamp `dur[dur < 0] = 0`, frames `(dur + 0.5).long()`
                      (csrc/ft_lr.hip: ft_gen_durations_kernel) -- in float32 / integer arithmetic, so exact
  lr_scan             the LengthRegulator's clamp, rounding and exclusive prefix sums (ft_lr_scan_kernel)
  check_tokens        bit 2 if the pad id 0 sits inside an item's length     (ft_check_tokens_lens_kernel)

No GPU, no project kernel.  The float functions work in float64; tests/test_lens_cpu.py proves them against torch's
float64 conv1d / layer_norm item by item, and the integer ones bit for bit against a per-item torch float32 evaluation.
The edge tables of tests/test_gpu_lens_kernels.py are the module constants at the end; test_lens_cpu.py asserts the
property that makes each row an edge.  Test-side only."""
import math

import numpy as np

U = 2.0 ** -24                      # one fp32 rounding, relative


def f64(t):
    """float64 numpy copy of a numpy array or a torch tensor (any device)"""
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def bf16_round(a):
    """float32 array rounded to the nearest bf16 (ties to even), as float32; finite values only"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def valid_rows(lens, T):
    """bool [B,T]: t < lens[b] (a length above T is T, one below 0 is 0)"""
    return np.arange(T)[None, :] < np.asarray(lens, dtype=np.int64)[:, None]


# ---- convolution with bias ------------------------------------------------------------------------------------------
def conv_bias_lens(x, w, bias, relu, lens, bf16=False):
    """x [B,T,Cin], w [Cout,Cin,k] (k odd), bias [Cout] -> (want, mag), float64 [B,T,Cout]:
    want[b,t,o] = act(bias[o] + sum_{j,c} x[b, t + j - k//2, c] * w[o,c,j]) at t < lens[b] and 0 past it, reads outside
    [0, T) being zero; mag = the same sum over absolute values + |bias| (0 past the length too).
    bf16: both operands are rounded to the nearest bf16 first (their products are then exact in fp32)."""
    if bf16:
        x, w = bf16_round(f64(x).astype(np.float32)), bf16_round(f64(w).astype(np.float32))
    x, w, bias = f64(x), f64(w), f64(bias)
    B, T, Cin = x.shape
    Cout, _, k = w.shape
    xp = np.zeros((B, T + 2 * k, Cin))
    xp[:, k:k + T] = x
    acc = np.zeros((B, T, Cout)) + bias
    mag = np.zeros((B, T, Cout)) + np.abs(bias)
    for j in range(k):
        seg = xp[:, k + j - k // 2:k + j - k // 2 + T]
        acc += seg @ w[:, :, j].T
        mag += np.abs(seg) @ np.abs(w[:, :, j]).T
    if relu:
        acc = np.maximum(acc, 0.0)
    keep = valid_rows(lens, T)[:, :, None]
    return np.where(keep, acc, 0.0), np.where(keep, mag, 0.0)


def conv_f32_bound(mag, Cin, k):
    """ft_gemm_rows_kernel (f32 MFMA: exact products, fp32 accumulator): the n = k * Cin products are accumulated in some
    order, n roundings at most, + 1 for the bias, + 1 spare: (n + 2) 2^-24 (sum|x||w| + |bias|)"""
    return (k * Cin + 2) * U * mag + 1e-30


def conv_b3_bound(mag, bias, Cin, k, bf16):
    """The bf16-split kernels of ft_gemm_b3.hip.  The accumulator is fp32 and takes at most one rounding per MFMA input
    product: 16 per v_mfma_f32_32x32x16_bf16, one MFMA per 16 k (K padded up) and tap in bf16 mode, six (the six kept
    terms of the three-way operand split) in fp32 mode, where the three dropped terms add <= 2^-23 |x||w| per product;
    + 1 rounding for the bias, + 1 spare.  mag = sum|x||w| + |bias|."""
    R = (1 if bf16 else 6) * 16 * k * math.ceil(Cin / 16) + 2
    dropped = 0.0 if bf16 else 2.0 ** -23 * np.maximum(mag - np.abs(f64(bias)), 0.0)
    return R * U * mag + dropped + 1e-30


# ---- add + LayerNorm -----------------------------------------------------------------------------------------------
def add_layernorm_lens(x, res, gamma, beta, lens, eps):
    """x, res (or None) [B,T,D] -> (want float64 [B,T,D]: LayerNorm(x + res) * gamma + beta at t < lens[b], 0 past it;
    smax [B,T] = max_c |s|, sigma [B,T] = sqrt(biased variance of s), xhat [B,T,D] = (s - mean) / sqrt(var + eps), of
    s = x + res -- what layernorm_bound needs).  eps is an fp32 argument of the C ABI: rounded to fp32 first."""
    eps = float(np.float32(eps))
    s = f64(x) if res is None else f64(x) + f64(res)
    B, T, D = s.shape
    keep = valid_rows(lens, T)
    s = np.where(keep[:, :, None], s, 0.0)                      # (rows past the length may hold NaN: never used)
    mu = s.mean(-1, keepdims=True)
    var = ((s - mu) ** 2).mean(-1, keepdims=True)
    xhat = (s - mu) / np.sqrt(var + eps)
    want = np.where(keep[:, :, None], xhat * f64(gamma) + f64(beta), 0.0)
    return want, np.abs(s).max(-1), np.sqrt(var[..., 0]), xhat


def layernorm_bound(want, smax, sigma, xhat, gamma, eps, D, has_res):
    """Forward error bound, per element, of a two-pass fp32 LayerNorm  y_c = (s_c - mu) * rs * gamma_c + beta_c  whose
    sums run over n = ceil(D / 64) + 6 additions per summand (a lane's sequential part, then a 6-step butterfly), every
    operation rounded once (u = 2^-24).  S = max_c |s_c|, se = sqrt(var + eps), xh_c = (s_c - mu) / se:

      s_c    = fl(x_c + res_c)                    |ds_c| <= u S              (0 without a residual; counted anyway)
      mu     = fl(fl(sum s) / D)                  |dmu|  <= n u S + u S + u |mu| <= (n + 2) u S
      d_c    = fl(s_c - mu)                       |dd_c| <= u S + (n + 2) u S + u |d_c| = E + u |d_c|,  E = (n + 3) u S
      v      = fl(fl(sum d_c^2) / D + eps)        sum (d + dd)^2 = sum d^2 + 2 sum d dd + sum dd^2, and with
                                                  sum |d_c| <= D sigma:  |dv| / (var + eps) <= 2 q + q^2 + (n + 5) u,
                                                  q = E / se  (2 u from 2 u |d_c| d_c, 1 for a square, n for the sum, 1 for
                                                  the division, 1 for + eps)
      rs     = fl(1 / fl(sqrt v))                 relative: q + q^2 / 2 + (n + 5) u / 2 + 4 u   (sqrt and division within
                                                  one ulp = 2 u each)
      h_c    = fl(d_c rs)                         |dh_c| <= E / se + u |xh_c| + |xh_c| (rel. error of rs) + u |xh_c|
                                                        =  q (1 + |xh_c|) + |xh_c| (q^2 / 2 + ((n + 5) / 2 + 6) u)
      y_c    = fl(fl(h_c gamma_c) + beta_c)       |dy_c| <= |gamma_c| (|dh_c| + u |xh_c|) + u |y_c|

    so  |err_c| <= |gamma_c| u [ (n + 3) (S / se) (1 + |xh_c|) (1 + q) + ((n + 5) / 2 + 7) |xh_c| ] + u |y_c|
    (q^2 / 2 |xh_c| <= q^2 (1 + |xh_c|); terms of order u^2 that do not carry S / se are dropped).  Any order of the
    additions inside the sums, a fused multiply-add or a Welford / cascade summation only removes roundings."""
    n = math.ceil(D / 64) + 6
    se = np.sqrt(sigma ** 2 + float(np.float32(eps)))[..., None]
    q = (n + 3) * U * smax[..., None] / se
    ax = np.abs(xhat)
    return np.abs(f64(gamma)) * U * ((n + 3) * (smax[..., None] / se) * (1 + ax) * (1 + q) + ((n + 5) / 2 + 7) * ax) \
        + U * np.abs(want) + 1e-30


# ---- transpose + pad -----------------------------------------------------------------------------------------------
def transpose_pad_lens(x, lens, Tout, pad):
    """x float32 [B,T,C] -> float32 [B,C,Tout]: out[b,c,t] = x[b,t,c] if t < min(max(lens[b], 0), T) else pad"""
    x = np.asarray(x, dtype=np.float32)
    B, T, C = x.shape
    out = np.full((B, C, Tout), np.float32(pad), dtype=np.float32)
    for b in range(B):
        L = min(max(int(lens[b]), 0), T, Tout)
        out[b, :, :L] = x[b, :L].T
    return out


# ---- durations ------------------------------------------------------------------------------------------------------
def _frames(v):
    """(dur + 0.5).long(): the addition in float32, truncation toward zero"""
    return np.trunc(np.asarray(v, dtype=np.float32) + np.float32(0.5)).astype(np.int64)


def gen_durations(dur_f32, x_len):
    """dur float32 [B,Tx], x_len [B] -> (dur_out float32 [B,Tx], mel_len int64 [B], bad int).  Per item, alone:
    L = clamp(x_len, 1, Tx), bad = 1 if any x_len was outside [1, Tx]; if sum_{j<L} trunc(dur[j]) <= 0 every token
    j < L gets 2.0, else max(dur[j], 0) (a -0.0 stays, as `dur[dur < 0] = 0` leaves it); tokens j >= L get 0 and are not
    read; mel_len = sum_j int64(float32(dur_out[j]) + float32(0.5))."""
    dur = np.asarray(dur_f32, dtype=np.float32)
    B, Tx = dur.shape
    out = np.zeros_like(dur)
    mel_len = np.zeros(B, dtype=np.int64)
    bad = 0
    for b in range(B):
        L = int(x_len[b])
        if L < 1 or L > Tx:
            bad = 1
            L = 1 if L < 1 else Tx
        d = dur[b, :L]
        if int(np.trunc(d).astype(np.int64).sum()) <= 0:
            out[b, :L] = np.float32(2.0)
        else:
            out[b, :L] = np.where(d < 0, np.float32(0.0), d)
        mel_len[b] = _frames(out[b]).sum()
    return out, mel_len, bad


def lr_scan(dur_f32):
    """dur float32 [B,Tx] -> (cum int32 [B,Tx+1]: exclusive prefix sums of the frames per token, total int32 [B]);
    negatives count as 0"""
    dur = np.asarray(dur_f32, dtype=np.float32)
    B, Tx = dur.shape
    r = _frames(np.where(dur < 0, np.float32(0.0), dur))
    cum = np.zeros((B, Tx + 1), dtype=np.int64)
    cum[:, 1:] = np.cumsum(r, axis=1)
    return cum.astype(np.int32), cum[:, Tx].astype(np.int32)


def check_tokens(idx, lens):
    """2 if any idx[b,t] == 0 at t < lens[b], else 0"""
    idx = np.asarray(idx)
    return 2 if bool(((idx == 0) & valid_rows(lens, idx.shape[1])).any()) else 0


# =====================================================================================================================
# edge tables of tests/test_gpu_lens_kernels.py (their properties: tests/test_lens_cpu.py)
# =====================================================================================================================
# ---- masked convolution: the tile geometry of test_gpu_generate_batch.py / test_gpu_generate_batch_paths.py ----------
# small: rows (b, t) = (row // 37, row % 37) in 64-row tiles -- item 1 ends ONE ROW BEHIND a boundary (its last valid row
# is the first row of tile 1), item 3 ends AT one (its first masked row is row 128); item 0 is full, item 2 one row.
# large: 5 * 2480 = 12400 rows >= 96 * 128 with Cout = 256 -> 128-row tiles: item 0 one row behind a boundary, item 1 at
# one, item 2 one row, item 3 full, item 4 ends inside a tile, in the second 32-row block of a wave.
T_SMALL, LENS_SMALL = 37, [37, 28, 1, 17]
T_BIG, LENS_BIG, COUT_BIG = 2480, [641, 720, 1, 2480, 1337], 256

# ---- add + LayerNorm -------------------------------------------------------------------------------------------------
LN_B, LN_T = 3, 11                        # 33 rows: not a multiple of the 4 rows of a block
LN_LENS = [11, 1, 6]
LN_LENS_EDGE = [0, 11, 12]                # an empty item, a length above T
LN_DIMS = [7, 64, 130, 384]               # fewer channels than a wave | exactly one pass | a ragged last pass (3rd, 6th)
LN_EPS = 1e-5


def layernorm_inputs(D, has_res, offset, seed=0):
    """(x, res or None, gamma, beta) float32 numpy; offset: + 100 on every row of x (a mean 100 spreads away is where a
    one-pass variance fails); beta of magnitude >= 0.5 so that a row normalised from zeros is visibly not 0"""
    g = np.random.default_rng(1000 * D + 10 * int(has_res) + int(offset) + seed)
    x = g.standard_normal((LN_B, LN_T, D)).astype(np.float32)
    if offset:
        x = (x + np.float32(100.0)).astype(np.float32)
    res = g.standard_normal((LN_B, LN_T, D)).astype(np.float32) if has_res else None
    gamma = (1.0 + 0.3 * g.standard_normal(D)).astype(np.float32)
    beta = (np.where(g.random(D) < 0.5, -1.0, 1.0) * (0.5 + g.random(D))).astype(np.float32)
    return x, res, gamma, beta


# ---- transpose + pad -------------------------------------------------------------------------------------------------
PAD = float(np.float32(math.log(1e-5)))   # -11.5129...: the models' padding_value, as the fp32 the C ABI gets
TP_SHAPES = [(1, 1, 1, 1), (3, 33, 31, 40), (2, 65, 80, 64), (2, 64, 64, 97)]      # (B, T, C, Tout)


def transpose_lens_sets(B, T):
    """lens vectors of B entries covering 0, 1, T, T + 3, a negative length and 31 / 32 / 33 around the 32-wide tile"""
    pool = [T, 0, 1, T + 3, -2, 31, 32, 33, T - 1]
    pool += [pool[i % len(pool)] for i in range((-len(pool)) % B)]
    return [pool[i:i + B] for i in range(0, len(pool), B)]


# ---- durations -------------------------------------------------------------------------------------------------------
DUR_TX = [1, 63, 64, 65, 130]             # one wave pass | the 64-token stride | the scan's carry across 64-token chunks
# exactly on the rounding edges: 0.49999997 = 0.5 - 2^-25 rounds UP to 1 through the fp32 sum 0.49999997 + 0.5 == 1.0;
# 0.99999994 = 1 - 2^-24 truncates to 0 but counts one frame; -0.0 is not < 0; the negatives truncate to -0 and clamp to 0
DUR_EDGES = [0.5, 1.0, 1.5, 0.49999997, 0.99999994, -0.0, -0.3, -0.9999]
JUNK = [float('nan'), 1e30]               # what the padding (j >= x_len[b]) holds


def _junk_tail(d, L):
    for j in range(max(L, 0), len(d)):
        d[j] = JUNK[j % 2]
    return d


def duration_table(Tx, in_range=False):
    """-> (names, dur float32 [B,Tx], x_len int64 [B]).  in_range: the three items with x_len 0, -3, Tx + 1 get the length
    they are treated as (1, 1, Tx), so that bad == 0."""
    g = np.random.default_rng(77 + Tx)
    f32 = np.float32
    items = []

    def add(name, d, L):
        d = np.asarray(d, dtype=f32).copy()
        assert d.shape == (Tx,)
        items.append((name, _junk_tail(d, min(max(L, 1), Tx)), L))

    def rnd():
        return (g.random(Tx) * 4.0 + 0.6).astype(f32)          # 0.6 .. 4.6: truncated sum > 0 whenever one is >= 1

    if Tx == 1:                             # one token per item: each edge value alone (truncated sum <= 0 -> fallback
        for v in DUR_EDGES + [0.6, 2.5]:    # for all but 1.0, 1.5 and 2.5)
            add(f'edge {v!r}', [v], 1)
    else:
        edges = np.resize(np.asarray(DUR_EDGES + [2.25, 3.7], dtype=f32), Tx)
        add('edges', edges, Tx)
        add('ordinary a', rnd() + f32(1.0), max(Tx - 5, 1))
        add('all 0.6', np.full(Tx, 0.6, dtype=f32), Tx - 2)                  # truncated sum 0, every rounded duration 1
        add('ordinary b', rnd() + f32(1.0), Tx)
        zero = np.full(Tx, 0.3, dtype=f32)
        zero[:4] = [1.5, -1.2, 0.7, -0.4]                                    # 1 - 1 + 0 - 0 == 0 -> fallback
        add('truncated sum 0', zero, Tx)
        one = zero.copy()
        one[0] = 2.5                                                         # 2 - 1 == 1 -> no fallback, negatives clamp
        add('truncated sum 1', one, Tx)
    lo = rnd()
    add('x_len 0', lo, 1 if in_range else 0)                                 # treated as length 1
    add('x_len -3', rnd() - f32(0.55), 1 if in_range else -3)                # (first token 0.05 .. 4.05)
    add('x_len Tx + 1', rnd(), Tx if in_range else Tx + 1)                   # treated as length Tx
    names = [n for n, _, _ in items]
    return names, np.stack([d for _, d, _ in items]), np.asarray([L for _, _, L in items], dtype=np.int64)


# ---- token check -----------------------------------------------------------------------------------------------------
TOK_B, TOK_T = 4, 300                     # 1200 ids: five 256-thread blocks
TOK_LENS = [300, 1, 257, 130]
