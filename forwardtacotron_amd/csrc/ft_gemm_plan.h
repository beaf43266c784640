// What a GEMM launch will be, decided on the host in plain C++ (no HIP header, no device code): the descriptors of the
// "rows" (NT / NN) and "TN" (weight-gradient) launches, and for each launch the kernel (FtGemmVariant), tile, split
// count, grid and scratch size it gets.  ft_gemm.hip / ft_gemm_b3.hip put the HIP calls around plan_rows / plan_tn;
// tests/test_gemm_plan_cpu.py and tests/cpp/gemm_plan_main.cpp hold them to a hand-written table without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

// logical row r = (b, t), b = r / Tlog, t = r % Tlog:
//   physical row = b*bstride + (t+shift)*tstride, valid iff 0 <= t+shift < Tvalid ; invalid rows read as zeros.
//   shift = shift0 + tap*shift_step.
// batch-major [B,Tbuf,C]: bstride = Tbuf, tstride = 1 ; time-major [T,B,C]: bstride = 1, tstride = B.
struct FtRowMap {
  int Tlog, bstride, tstride, Tvalid, shift0, shift_step;
};

static inline FtRowMap ft_rowmap_identity(int rows) {
  int n = rows > 0 ? rows : 1;
  FtRowMap m = {n, 0, 1, n, 0, 0};
  return m;
}
// rows = B*T logical (b,t) positions stored time-major ([T,B,C]) when tm_B > 0, else plain row-major
static inline FtRowMap ft_rowmap_layout(int rows, int tm_B) {
  if (tm_B <= 0) return ft_rowmap_identity(rows);
  int T = rows / tm_B;
  FtRowMap m = {T > 0 ? T : 1, 1, tm_B, T, 0, 0};
  return m;
}

// C[cmap(M),N] (+)= sum_{tap} Amap_tap(A)[M,K] * B_tap   (+bias, relu, affine)
//   B_NCONTIG = false: B_tap[n][k] at B + tap*b_tap_stride + n*ldb + k   ("NT")
//   B_NCONTIG = true : B_tap[k][n] at B + tap*b_tap_stride + k*ldb + n   ("NN")
struct FtGemmTask {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* scale;   // optional per-column affine applied AFTER relu (eval-mode BatchNorm fold)
  const float* shift;
  long lda, ldb, ldc, b_tap_stride;
  int M, N, K, taps;
  FtRowMap amap;
  FtRowMap cmap;        // output row permutation (Tlog/bstride/tstride only); identity by default
  int relu, accumulate, a_vec, b_vec;
  // NN form only: every row of A is readable up to the next multiple of 4 of K (values there are ignored), so a K that
  // is not a multiple of 4 can still take the 16-B-load path
  int a_rowpad;
  // strided batch (attention: one GEMM per (batch item, head)); only for single-task launches.
  // instance z = blockIdx.z -> (z0, z1) = (z / nz1, z % nz1); X += z0*sX0 + z1*sX1 (floats)
  int nz, nz1;
  long sA0, sA1, sB0, sB1, sC0, sC1;
  // BatchNorm statistics from the epilogue (128x128 bf16-split kernel only; see ft_launch_gemm_rows): per M-tile and
  // column, (sum, sum of squares) of the stored values (after bias / ReLU) over the tile's rows with t = row % amap.Tlog
  // < stat_tvalid, as doubles at stat[((long)mtile * stat_ld + stat_col0 + col) * 2 + {0,1}] -- the layout of the
  // chunked partials ft_bn.hip finalizes.  stat = null: off.
  double* stat;
  int stat_ld, stat_col0, stat_tvalid;
};
#define FT_MAX_TASKS 16
struct FtGemmBatch {
  FtGemmTask t[FT_MAX_TASKS];
  // chain > 1: tasks 0..chain-1 are ONE product, accumulated in registers: C = sum_i sum_tap shift(A_i) * B_i,tap with
  // task 0's M, N, output and epilogue (conv-bank data gradient: every member adds into the same dx)
  int chain;
  int stat_fused;       // out: 1 if the launched kernel produced the tasks' BatchNorm statistics
  // Highway epilogues (HighwayNetwork, common_layers.py:35-40) of a single-task or chained launch with identity output
  // rows -- the north-star's "Highway fused": the gate never runs as a kernel of its own.
  //  hw_mode 1 (forward): B is the 32-row interleave of W1 / W2 (ft_highway_pack), N = 2 * hw_C; output column n is unit
  //    (n / 64) * 32 + n % 32 of y1 (n % 64 < 32) or of y2, so a wave's two 32-column tiles -- or, in the 64-column
  //    tiling, the two waves of a tile row -- hold y1 and y2 of the same units.  The epilogue writes
  //    out = g * relu(y1) + (1 - g) * x, g = sigmoid(y2), to C (ldc) and, if hw_x12 is set, the pre-activations
  //    [M, 2 * hw_C] = y1 | y2 (what the backward needs).  Biases hw_b1 / hw_b2 (task bias unused).
  //  hw_mode 2 (backward): the product (+ C when accumulate is set) is d(out) of the layer BELOW the one whose data
  //    gradient is being formed; the epilogue turns it into that layer's gate gradients at once:
  //    hw_d12 [M, 2 * hw_C] = d * g * (y1 > 0) | d * (relu(y1) - x) * g * (1 - g),  C = d * (1 - g)  (y1 | y2 = hw_x12).
  // ReLU gradient mask in the epilogue (single-task / chained launches, identity output rows): C = (product) where
  // relu_mask[row * ldc + col] > 0, else 0 -- the data gradient of a convolution that follows a conv + ReLU goes straight
  // through that ReLU's derivative (FFTBlock conv2 -> conv1, common_layers.py:178-180), no element-wise pass in between
  const float* relu_mask;
  // force_tile: 0 = the launcher picks the tile (and with it the kernel: 128x128 bf16-split or 64x64 f32) from the
  // launch's own size; 1 = 64, 2 = 128 -- a GEMM issued in row chunks then rounds exactly like the same GEMM issued
  // whole (ft_*_layer_fwd; gemm_plan::tiles_big gives the whole launch's choice)
  int force_tile;
  // Split-K of a single-task or chained NT launch with FEW output tiles and a LONG contraction (the token-side data
  // gradients: 4,096 rows): ksplit_slab != null offers ft_rows_ksplit_floats() floats of scratch; the launcher then may cut
  // the stage sequence into ksplit ranges (grid z), every range writing its raw partial tile to slab[z][M][N], and a second
  // launch adds the partials in range order and applies bias / accumulate / the output row map.  ksplit is set by the
  // launcher (0 / 1: not split).  Sums the same products in another order than the unsplit launch: callers are gradients.
  float* ksplit_slab;
  int ksplit;
  int hw_mode, hw_C;
  const float* hw_x;
  const float* hw_b1;
  const float* hw_b2;
  float* hw_x12;
  float* hw_d12;
  // Row mask in the epilogue (the length-aware eval convolutions, ft_conv1d_fwd_lens): int64 [items] or null.  A stored
  // row (item, t) = (row / amap.Tlog, row % amap.Tlog) of any task with t >= out_lens[item] is written as exactly 0,
  // whatever bias / ReLU / scale-shift / accumulate would have made of it.  Not combined with split-K or the highway modes.
  const long* out_lens;
};
static_assert(sizeof(FtGemmBatch) <= 4080, "FtGemmBatch travels as a kernel argument (4 KB limit)");

// out_tap[m][n] = sum_r Amap(A)[r][m] * Bmap_tap(B)[r][n],  r over R logical rows   ("TN", split over rows)
// result written to dst[m*ldm + n*ldn + tap*ldj]  (deterministic slab + reduce)
struct FtGemmTNTask {
  const float* A;
  const float* B;
  float* dst;
  long lda, ldb;
  long ldm, ldn, ldj;
  int M, N, R, taps;
  FtRowMap amap, bmap;
  int a_vec, b_vec, accumulate;
  // rows of A / B are readable up to the next multiple of 4 of M / N (those columns only reach masked outputs)
  int rowpad;
  // strided batch (see FtGemmTask); dst += z0*sD0 + z1*sD1
  int nz, nz1;
  long sA0, sA1, sB0, sB1, sD0, sD1;
  // conv-bank mode (bankC > 0): A's M columns are the K = M / bankC members of a CBHG conv bank side by side, member
  // kk = m / bankC + 1 has kernel size kk: tap j < kk only, B row shift j - kk/2, A rows t < (kk odd ? bankTodd :
  // amap.Tvalid); the result goes to bank_dst[kk-1] in torch layout [bankC][N][kk].  bankC % tile == 0.
  int bankC, bankTodd;
  float* bank_dst[FT_MAX_TASKS];
};

// Which kernel each GEMM launch took, counted on the host at the dispatch sites since the library loaded
// (ft_gemm_variant_counts; the order is the ABI's, include/fwdtaco_hip.h).  Plain integers: no device work, no
// synchronisation.  Tests assert the delta of the one variant they mean to exercise, so a planner threshold that moves
// a test's shape onto another kernel fails that test instead of quietly testing less.
enum FtGemmVariant {
  FT_GV_ROWS_F32_64_NT_FAST = 0, FT_GV_ROWS_F32_64_NT_SLOW, FT_GV_ROWS_F32_64_NN_FAST, FT_GV_ROWS_F32_64_NN_SLOW,
  FT_GV_ROWS_F32_128_NT_FAST, FT_GV_ROWS_F32_128_NT_SLOW, FT_GV_ROWS_F32_128_NN_FAST, FT_GV_ROWS_F32_128_NN_SLOW,
  FT_GV_ROWS_B3_64, FT_GV_ROWS_B3_128, FT_GV_ROWS_B3P, FT_GV_ROWS_B3P_KSPLIT,
  FT_GV_TN_F32_64_FAST, FT_GV_TN_F32_64_SLOW, FT_GV_TN_F32_128_FAST, FT_GV_TN_F32_128_SLOW,
  FT_GV_TN_B3_64, FT_GV_TN_B3_128, FT_GV_TN_B3P,
  FT_GV_COUNT
};

namespace gemm_plan {

constexpr int BK = 32;           // contraction depth of one stage of the f32 kernels (ft_gemm.hip asserts the equality)
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// The FT_GEMM_* / FT_TN_* switches, A/B knobs and tuning aids.  env = getenv in the library, which fills ONE instance on
// first use (they are per-process, never per-launch); any table in a test.
struct Switches {
  int b3;          // FT_GEMM_B3=0: no launch takes the bf16-split (exact 3-way operand split) kernels in fp32 mode
  int b3_tn;       // FT_GEMM_B3_TN: 0 = weight gradients never take the bf16-split path, 1 = every tile size does (value 2),
                   // default (value 1): 128x128 only
  int ksplit;      // FT_GEMM_KSPLIT=0: never split K of a rows launch
  int pipe;        // FT_GEMM_PIPE=0: the two-barrier 128x128 rows kernel instead of the pipelined one
  int tn_pipe;     // FT_GEMM_TN_PIPE=0: the two-barrier 128x128 TN kernel instead of the pipelined one
  long tn_force_s; // FT_TN_FORCE_S=<n>: tuning aid (lab/tn_split_lab.py)
  int log;         // FT_GEMM_LOG=1: every launch timed and logged (tools/gemm_report.py)
  explicit Switches(const char* (*env)(const char*)) {
    auto get = [&](const char* name) { return env ? env(name) : nullptr; };
    auto not0 = [&](const char* name) {
      const char* e = get(name);
      return (e && e[0] == '0') ? 0 : 1;
    };
    b3 = not0("FT_GEMM_B3");
    const char* e = get("FT_GEMM_B3_TN");
    b3_tn = e ? (e[0] == '1' ? 2 : (e[0] == '0' ? 0 : 1)) : 1;
    ksplit = not0("FT_GEMM_KSPLIT");
    pipe = not0("FT_GEMM_PIPE");
    tn_pipe = not0("FT_GEMM_TN_PIPE");
    e = get("FT_TN_FORCE_S");
    tn_force_s = e ? atol(e) : 0L;
    e = get("FT_GEMM_LOG");
    log = (e && e[0] == '1') ? 1 : 0;
  }
  int tn_b3_mode() const { return b3 ? b3_tn : 0; }
};

// 16-byte loads from an operand: aligned base, and every stride that moves the base a multiple of 4 floats
inline int vec_ok(const float* p, long ld, long s0, long s1, long s2 = 0) {
  return ld % 4 == 0 && ((uintptr_t)p) % 16 == 0 && s0 % 4 == 0 && s1 % 4 == 0 && s2 % 4 == 0;
}

// the defaulting every rows launch gets: identity output rows, one instance, the chain flag, a_vec / b_vec, and task 0
// in the unused slots (the kernels index t[] with a uniform but unchecked task id)
inline void normalise(FtGemmBatch& b, int ntasks) {
  for (int i = 0; i < ntasks; ++i) {
    FtGemmTask& t = b.t[i];
    if (t.cmap.Tlog <= 0) t.cmap = ft_rowmap_identity(t.M);     // tasks built with memset(0): identity output
    if (t.nz <= 1) {
      t.nz = t.nz1 = 1;
      t.sA0 = t.sA1 = t.sB0 = t.sB1 = t.sC0 = t.sC1 = 0;
    }
    t.a_vec = vec_ok(t.A, t.lda, t.sA0, t.sA1);
    t.b_vec = vec_ok(t.B, t.ldb, t.sB0, t.sB1, t.b_tap_stride);
  }
  for (int i = ntasks; i < FT_MAX_TASKS; ++i) b.t[i] = b.t[0];
  if (b.chain <= 1) b.chain = 0;
}
inline void normalise(FtGemmTNTask& t) {
  if (t.nz <= 1) {
    t.nz = t.nz1 = 1;
    t.sA0 = t.sA1 = t.sB0 = t.sB1 = t.sD0 = t.sD1 = 0;
  }
  t.a_vec = vec_ok(t.A, t.lda, t.sA0, t.sA1);
  t.b_vec = vec_ok(t.B, t.ldb, t.sB0, t.sB1);
}

// ------------------------------------------------------------------------------------------------------------------
// rows (NT / NN) launches

// the tile choice for a launch whose tasks have `tiles128` 128x128 output tiles in total (callers that issue one GEMM
// in row chunks pre-decide FtGemmBatch.force_tile with the whole GEMM's numbers)
inline bool tiles_big(long tiles128, int maxM, int maxN) { return tiles128 >= 192 && maxN > 64 && maxM > 64; }

// may these tasks take the pipelined 128x128 kernel (the only one that implements split-K)?
inline bool rows_pipe_ok(const FtGemmBatch& b, int ntasks, const Switches& sw) {
  // the pipelined kernel addresses a tile's rows with 32-bit byte offsets from the tile's first row (buffer loads)
  bool span_ok = true;
  for (int i = 0; i < (b.t[0].nz > 1 ? 1 : ntasks) && i < FT_MAX_TASKS; ++i) {
    const FtGemmTask& t = b.t[i];
    const long tl = t.amap.Tlog, ts = t.amap.tstride, bs = t.amap.bstride;
    const long rows = (tl < 128 ? tl : 128) * ts + (128 / tl + 2) * bs + tl * ts;     // bound on a tile's physical row span
    span_ok = span_ok && ts >= 0 && bs >= 0 && rows * t.lda * 4 < (1L << 31) && 128L * t.ldb * 4 < (1L << 31);
  }
  return sw.pipe && span_ok;
}

// Split-K ranges of an NT launch that was offered scratch (FtGemmBatch.ksplit_slab), from its shape alone; 1: not split.
// Only single-task / chained products with few 128x128 output tiles, a long stage sequence (>= 128 stages of 16 k) and a
// plain epilogue; S ranges of >= 32 stages each, S * tiles <= the stream's slots.  The scratch queries call this: they
// have no operands yet, so what they answer is the offer a launch with 16-byte-aligned fp32 operands takes up.
inline int rows_ksplit(const FtGemmBatch& b, int ntasks, long slots, const Switches& sw) {
  const bool chained = b.chain > 1;
  if (!sw.ksplit || !(chained ? b.chain == ntasks : ntasks == 1) || !sw.b3) return 1;
  const FtGemmTask& t0 = b.t[0];
  if (t0.nz > 1 || t0.relu || t0.scale || t0.stat || b.hw_mode || b.relu_mask || b.out_lens || t0.N % 4 != 0 ||
      t0.M <= 64 || t0.N <= 64)
    return 1;
  if (!rows_pipe_ok(b, ntasks, sw)) return 1;
  long stages = 0;
  for (int i = 0; i < ntasks; ++i) stages += (long)b.t[i].taps * cdiv(b.t[i].K, 16);
  const long tiles = (long)cdiv(t0.M, 128) * cdiv(t0.N, 128);
  if (stages < 128) return 1;                      // (a short contraction gains nothing: launch + second pass)
  long S = slots / (tiles > 0 ? tiles : 1);
  if (S > stages / 32) S = stages / 32;
  if (S > 16) S = 16;
  if (S < 2) return 1;
  const long per = (stages + S - 1) / S;
  return (int)((stages + per - 1) / per);            // no empty range
}
inline size_t rows_ksplit_floats(const FtGemmBatch& b, int ntasks, long slots, const Switches& sw) {
  const int S = rows_ksplit(b, ntasks, slots, sw);
  return S > 1 ? (size_t)S * b.t[0].M * b.t[0].N : 0;
}

struct RowsPlan {
  int variant;                 // FtGemmVariant
  bool big, fast, b3;          // 128x128 tile; 16-byte loads; the bf16 matrix pipe (3 planes, or 1 in bf16 precision)
  int ksplit;                  // 0: not split
  size_t ksplit_floats;
  int stat_fused;
  int grid[3];                 // grid[0] == 0 or grid[1] == 0: nothing to launch
};

// b: normalised.  precision: 0 = fp32-exact, 1 = bf16 operands / fp32 accumulate on every NT-form fast launch.
// slots: workgroup slots (2 per usable CU) of the launch's stream.
inline RowsPlan plan_rows(const FtGemmBatch& b, int ntasks, bool b_ncontig, int precision, long slots,
                          const Switches& sw) {
  RowsPlan p = {};
  const bool chained = b.chain > 1;
  int maxM = 0, maxN = 0;
  long tiles128 = 0;
  bool fast = true, vec = true;
  for (int i = 0; i < ntasks; ++i) {
    const FtGemmTask& t = b.t[i];
    if (t.M > maxM) maxM = t.M;
    if (t.N > maxN) maxN = t.N;
    tiles128 += (long)cdiv(t.M, 128) * cdiv(t.N, 128) * t.nz;
    const bool k_ok = t.K % 4 == 0 || (b_ncontig && t.a_rowpad && t.lda >= ((t.K + 3) & ~3));
    fast = fast && t.a_vec && t.b_vec && k_ok && (!b_ncontig || t.N % 4 == 0);
    vec = vec && t.a_vec && t.b_vec && t.K % 4 == 0;
  }
  if (chained) tiles128 /= ntasks;
  p.fast = fast;
  p.big = b.force_tile ? b.force_tile == 2 : tiles_big(tiles128, maxM, maxN);
  if (b.ksplit_slab && !b_ncontig && precision == 0 && vec) {
    const int S = rows_ksplit(b, ntasks, slots, sw);
    if (S > 1) {
      p.ksplit = S;
      p.ksplit_floats = (size_t)S * b.t[0].M * b.t[0].N;
      p.big = true;
    }
  }
  const int bm = p.big ? 128 : 64;
  p.grid[0] = cdiv(maxM, bm);
  p.grid[1] = cdiv(maxN, bm);
  p.grid[2] = p.ksplit > 1 ? p.ksplit : chained ? 1 : (ntasks == 1 ? b.t[0].nz : ntasks);
  // the 64x64 tile gains nothing from the split path (its staging per MFMA is twice the 128-tile's): f32 kernel there
  // bf16 precision mode: every NT-form fast launch takes the (one-plane) bf16 kernel, whatever its tile
  p.b3 = fast && !b_ncontig && ((p.big && sw.b3) || precision == 1);
  p.stat_fused = p.b3 && p.big && !chained;        // only the 128x128 split kernel computes BatchNorm statistics
  if (p.b3) {
    const bool piped = p.big && rows_pipe_ok(b, ntasks, sw);
    p.variant = piped ? (p.ksplit > 1 ? FT_GV_ROWS_B3P_KSPLIT : FT_GV_ROWS_B3P) : (p.big ? FT_GV_ROWS_B3_128 : FT_GV_ROWS_B3_64);
  } else {
    p.variant = (p.big ? FT_GV_ROWS_F32_128_NT_FAST : FT_GV_ROWS_F32_64_NT_FAST) + (b_ncontig ? 2 : 0) + (fast ? 0 : 1);
  }
  return p;
}

// ------------------------------------------------------------------------------------------------------------------
// TN (weight-gradient) launches

// the pipelined TN kernel addresses rows with 31-bit byte offsets from the operand's base (buffer loads) and walks them
// with non-negative strides
inline bool tn_span_ok(const FtRowMap& m, long R, long ld, int taps) {
  if (m.bstride < 0 || m.tstride < 0) return false;
  const long items = (R + m.Tlog - 1) / m.Tlog;
  long hi = m.shift0 > 0 ? m.shift0 : 0;
  const long last = (long)m.shift0 + (long)(taps - 1) * m.shift_step;
  hi = last > hi ? last : hi;
  hi += taps;                                    // conv-bank mode: shifts tap - kk/2 within [-taps, taps]
  // (rows below the base only occur masked, t + shift < 0: no lower bound needed)
  const long maxrow = (items + 1) * m.bstride + (m.Tlog + 16 + hi) * m.tstride;
  return (maxrow + 1) * ld * 4 + 1024 < (1L << 31);
}

enum TnReduce { TN_REDUCE_PLAIN, TN_REDUCE_TAP, TN_REDUCE_BANK };
struct TnPlan {
  int variant;                 // FtGemmVariant
  int tm;                      // tile = 64 * tm squared
  bool fast, b3, pipelined;
  int S, rows_per_split;
  size_t need_floats;          // S slabs of taps * nz * M * N
  int grid[3];
  TnReduce reduce;             // the launch that sums the slabs
};

// t: normalised (the workspace queries set a_vec / b_vec themselves: they have no operands yet)
inline TnPlan plan_tn(const FtGemmTNTask& t, int precision, long slots, const Switches& sw) {
  TnPlan p = {};
  const bool m_ok = t.M % 4 == 0 || (t.rowpad && t.lda >= ((t.M + 3) & ~3));
  const bool n_ok = t.N % 4 == 0 || (t.rowpad && t.ldb >= ((t.N + 3) & ~3));
  p.fast = t.a_vec && t.b_vec && m_ok && n_ok;
  // Tile and split count.  Split path usable (aligned operands): its 128x128 tile runs ~1.35x the f32 kernels' rate, so
  // it is preferred whenever tiles x split-K can still fill the chip -- the extra slabs it needs cost a few microseconds
  // of HBM traffic
  const int nz = t.nz > 1 ? t.nz : 1;
  long maxs = (t.R + 4 * BK - 1) / (4 * BK);      // at least 128 rows per split
  if (maxs < 1) maxs = 1;
  const long tiles128 = (long)cdiv(t.M, 128) * cdiv(t.N, 128) * t.taps * nz;
  bool small = tiles128 < 64 || t.M <= 64 || t.N <= 64;
  // ... as long as every split still has >= 1024 rows to amortise its prologue and its slab
  if (p.fast && sw.tn_b3_mode() >= 1 && t.M > 64 && t.N > 64 && tiles128 * (t.R / 1024) >= 256) small = false;
  p.tm = small ? 1 : 2;
  const int bm = 64 * p.tm;
  long tiles = (long)cdiv(t.M, bm) * cdiv(t.N, bm) * t.taps * nz;
  long want = tiles >= slots ? 1 : (slots + tiles - 1) / tiles;
  // the split-path kernel holds exactly 2 workgroups per CU (53 KB LDS, 220 VGPRs) = 512 slots: a grid slightly above
  // one full wave pays a second, nearly empty one (576 workgroups ran at 94 TF, 512 at 134) -> round DOWN there
  const bool split_path = p.fast && sw.tn_b3_mode() >= 1 && p.tm == 2;
  if (split_path && tiles < slots) want = slots / tiles;
  if (t.bankC > 0) {
    // conv-bank mode: member kk only has taps j < kk, i.e. (K+1)/(2K) of the grid does work; aim for ~4 waves of
    // workgroups so that the last, partial wave costs little
    const long K = t.taps;
    const long live = tiles * (K + 1) / (2 * K);
    want = (4 * slots + live - 1) / (live > 0 ? live : 1);
  }
  if (sw.tn_force_s > 0) want = sw.tn_force_s;
  long S = want < maxs ? want : maxs;
  if (S > 65535 / ((long)t.taps * nz)) S = 65535 / ((long)t.taps * nz);
  if (S < 1) S = 1;
  long rps = (t.R + S - 1) / S;
  rps = ((rps + BK - 1) / BK) * BK;
  if (rps < BK) rps = BK;
  S = (t.R + rps - 1) / rps;
  if (S < 1) S = 1;
  p.S = (int)S;
  p.rows_per_split = (int)rps;
  p.need_floats = (size_t)p.S * t.taps * nz * t.M * t.N;
  p.grid[0] = cdiv(t.M, bm);
  p.grid[1] = cdiv(t.N, bm);
  p.grid[2] = p.S * t.taps * nz;
  if (t.bankC > 0) {                               // live (member, tap, tile) triples along x (ft_tn_who)
    p.grid[0] = (t.bankC / bm) * (t.taps * (t.taps + 1) / 2);
    p.grid[2] = p.S;
  }
  // bf16-split TN form (r-pair packed LDS tiles, ft_gemm_b3.hip): on by default for the 128x128 tile; the 64x64 tile
  // has twice the staging per MFMA and stays on the f32 kernel unless FT_GEMM_B3_TN=1
  const int mode = sw.tn_b3_mode();
  p.b3 = p.fast && (precision == 1 || mode == 2 || (mode == 1 && p.tm == 2));
  // short splits (few stages per workgroup) do not amortise the deeper prologue: 256 x 256 x 26912 at 224 rows per split
  // ran 54 -> 59 us on the pipelined kernel, the shapes with >= 1000 rows per split gain 17-25 % (lab/tn_pipe_ab.py)
  p.pipelined = p.b3 && p.tm == 2 && sw.tn_pipe && p.rows_per_split % 16 == 0 && p.rows_per_split >= 512 &&
                t.amap.Tlog == t.bmap.Tlog && t.amap.Tlog >= 16 && tn_span_ok(t.amap, t.R, t.lda, t.taps) &&
                tn_span_ok(t.bmap, t.R, t.ldb, t.taps);
  if (p.b3) p.variant = p.pipelined ? FT_GV_TN_B3P : (p.tm == 2 ? FT_GV_TN_B3_128 : FT_GV_TN_B3_64);
  else p.variant = (p.tm == 2 ? FT_GV_TN_F32_128_FAST : FT_GV_TN_F32_64_FAST) + (p.fast ? 0 : 1);
  p.reduce = t.bankC > 0 ? TN_REDUCE_BANK : (t.taps * p.S <= 16 ? TN_REDUCE_PLAIN : TN_REDUCE_TAP);
  return p;
}

// the slabs a scratch query answers: it does not know the operands yet, so the larger of the plan of unaligned operands
// and the plan of aligned ones with padded rows, one of which the launcher will make
inline size_t tn_query_floats(const FtGemmTNTask& task, const Switches& sw) {
  FtGemmTNTask t = task;
  normalise(t);
  t.a_vec = t.b_vec = 0;
  const size_t slow = plan_tn(t, 0, 512, sw).need_floats;
  t.a_vec = t.b_vec = t.rowpad = 1;
  t.lda = t.lda > t.M + 3 ? t.lda : t.M + 3;
  t.ldb = t.ldb > t.N + 3 ? t.ldb : t.N + 3;
  const size_t fast = plan_tn(t, 0, 512, sw).need_floats;
  return slow > fast ? slow : fast;
}

// the weight gradients of nn.Linear and of a channels-last Conv1d as TN tasks (the C entry points and their scratch
// queries build the same task: the query with null operands and the dense leading dimensions)
inline FtGemmTNTask linear_wgrad_task(const float* dy, long lddy, const float* x, long ldx, float* dw, int rows, int in_f,
                                      int out_f, int B, int T, int x_shift, int accumulate, int dy_tm, int x_tm) {
  FtGemmTNTask t;
  memset(&t, 0, sizeof(t));
  t.A = dy; t.B = x; t.dst = dw;
  t.lda = lddy; t.ldb = ldx;
  t.ldm = in_f; t.ldn = 1; t.ldj = 0;
  t.M = out_f; t.N = in_f; t.R = rows; t.taps = 1;
  if (x_shift == 0 && !dy_tm && !x_tm) {
    t.amap = ft_rowmap_identity(rows);
    t.bmap = ft_rowmap_identity(rows);
  } else {          // both maps share the logical (b, t) decomposition with Tlog = T
    int Tl = T > 0 ? T : 1;
    FtRowMap am = {Tl, dy_tm ? 1 : Tl, dy_tm ? B : 1, Tl, 0, 0};
    FtRowMap bm = {Tl, x_tm ? 1 : Tl, x_tm ? B : 1, Tl, x_shift, 0};
    t.amap = am;
    t.bmap = bm;
  }
  t.accumulate = accumulate;
  return t;
}
inline FtGemmTNTask conv_wgrad_task(const float* dy, long lddy, const float* x, long ldx, float* dw, int B, int T, int Cin,
                                    int Cout, int k, int Tbuf, int Tvalid) {
  FtGemmTNTask t;
  memset(&t, 0, sizeof(t));
  t.A = dy; t.B = x; t.dst = dw;
  t.lda = lddy; t.ldb = ldx;
  t.ldm = (long)Cin * k; t.ldn = k; t.ldj = 1;       // torch layout [Cout][Cin][k]
  t.M = Cout; t.N = Cin; t.R = B * Tvalid; t.taps = k;
  int Tl = Tvalid > 0 ? Tvalid : 1;
  FtRowMap am = {Tl, Tbuf, 1, Tvalid, 0, 0};
  FtRowMap bm = {Tl, T, 1, T, -(k / 2), 1};
  t.amap = am;
  t.bmap = bm;
  return t;
}
inline size_t linear_wgrad_query_bytes(int rows, int in_f, int out_f, const Switches& sw) {
  return tn_query_floats(linear_wgrad_task(nullptr, out_f, nullptr, in_f, nullptr, rows, in_f, out_f, 1, rows, 0, 0, 0, 0),
                         sw) * sizeof(float);
}
inline size_t conv_wgrad_query_bytes(int B, int T, int Cin, int Cout, int k, int Tvalid, const Switches& sw) {
  return tn_query_floats(conv_wgrad_task(nullptr, Cout, nullptr, Cin, nullptr, B, T, Cin, Cout, k, Tvalid, Tvalid), sw) *
         sizeof(float);
}

}  // namespace gemm_plan
