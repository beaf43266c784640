// Stand-alone host test of csrc/ft_gemm_plan.h (tests/test_gemm_plan_cpu.py builds it with the sanitizers and runs it):
// the kernel, tile, split and grid every kind of GEMM launch gets, against a hand-written table, plus the conditions
// every plan must meet over a sweep of shapes.
//
// Where the table comes from (never from the header under test):
//   variants    -- tests/test_gpu_gemm_edges.py asserts them on the GPU by launch counter (same shapes, leading dimensions
//                  and alignments), bench.py names the benchmark's; the switch rows follow from what each switch says
//   S, ksplit   -- the answers of the library's host-only workspace queries (ft_linear_bwd_weight_workspace /
//                  ft_linear_bwd_data_multi_workspace / ft_bgemm_tn_workspace / ft_conv_bank_bwd_weight_workspace) before
//                  the planner moved into the header; a query covers the aligned and the unaligned plan with the larger
//                  S, where the table has the smaller one it is worked out in the row's comment
//   rows_per_split = R / S rounded up, then up to a multiple of 32;  grid = output tiles x (S x taps | tasks | ksplit)
//   threshold rows -- test_rows_boundaries / test_tn_boundaries: what the launchers' own code gave at and beside every
//                  threshold before the planner moved here
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "ft_gemm_plan.h"

using namespace gemm_plan;

static int g_failed = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                               \
    }                                                           \
  } while (0)

// ---- switch tables ---------------------------------------------------------------------------------------------------
static const char* g_env_name = nullptr;
static const char* g_env_value = nullptr;
static const char* one_env(const char* name) { return g_env_name && !strcmp(name, g_env_name) ? g_env_value : nullptr; }
static Switches with(const char* name, const char* value) {
  g_env_name = name;
  g_env_value = value;
  return Switches(one_env);
}
static Switches defaults() { return with(nullptr, nullptr); }

// ---- operands: addresses are never dereferenced by the planner, only tested for alignment -----------------------------
static float* addr(int mis_floats = 0) { return reinterpret_cast<float*>(uintptr_t(0x100000 + 4 * mis_floats)); }

// ---- tasks as the C entry points build them (ft_capi_core.hip) --------------------------------------------------------
static FtGemmBatch zero_batch() {
  FtGemmBatch b;
  memset(&b, 0, sizeof(b));
  return b;
}
// ft_linear_fwd: y = x w^T, x rows ldx apart (base `mis` floats off 16 bytes), either side time-major over tm_B items
static FtGemmBatch linear_fwd(int rows, int in_f, int out_f, long ldx, int x_tm_B = 0, int y_tm_B = 0, int mis = 0) {
  FtGemmBatch b = zero_batch();
  FtGemmTask& t = b.t[0];
  t.A = addr(mis); t.B = addr(); t.C = addr(1);
  t.lda = ldx; t.ldb = in_f; t.ldc = out_f + 9;
  t.M = rows; t.N = out_f; t.K = in_f; t.taps = 1;
  t.amap = ft_rowmap_layout(rows, x_tm_B);
  t.cmap = ft_rowmap_layout(rows, y_tm_B);
  return b;
}
// ft_linear_bwd_data_multi(_ws): dx = sum_i dy_i w_i, n tasks chained (n > 1); slab: scratch for split-K offered
static FtGemmBatch data_multi(int n, int rows, int in_f, int out_f, long lddy, bool w_transposed, bool slab, int dx_tm_B = 0) {
  FtGemmBatch b = zero_batch();
  for (int i = 0; i < n; ++i) {
    FtGemmTask& t = b.t[i];
    t.A = addr(); t.B = addr(); t.C = addr(1);
    t.lda = lddy; t.ldb = w_transposed ? out_f : in_f; t.ldc = in_f + 9;
    t.M = rows; t.N = in_f; t.K = out_f; t.taps = 1;
    t.amap = ft_rowmap_identity(rows);
    t.cmap = ft_rowmap_layout(rows, dx_tm_B);
  }
  b.chain = n > 1 ? n : 0;
  if (slab) b.ksplit_slab = addr();
  return b;
}
// ft_bgemm_nn: C = A [M, K] B [K, N], one instance
static FtGemmBatch bgemm_nn(int M, int N, int K, long lda, int a_rows_padded) {
  FtGemmBatch b = zero_batch();
  FtGemmTask& t = b.t[0];
  t.A = addr(); t.B = addr(); t.C = addr(1);
  t.lda = lda; t.ldb = N; t.ldc = N + 9;
  t.M = M; t.N = N; t.K = K; t.taps = 1;
  t.amap = ft_rowmap_identity(M);
  t.a_rowpad = a_rows_padded;
  t.nz = t.nz1 = 1;
  return b;
}
// conv_fwd_task: channels-last Conv1d, tap-major weights
static void conv_fwd_task(FtGemmTask& t, long ldx, int B, int T, int Cin, int Cout, int k, int Tout) {
  memset(&t, 0, sizeof(t));
  t.A = addr(); t.B = addr(); t.C = addr(1);
  t.lda = ldx; t.ldb = Cin; t.ldc = Cout + 9; t.b_tap_stride = (long)Cout * Cin;
  t.M = B * Tout; t.N = Cout; t.K = Cin; t.taps = k;
  FtRowMap m = {Tout > 0 ? Tout : 1, T, 1, T, -(k / 2), 1};
  t.amap = m;
}
static FtGemmBatch conv_fwd(long ldx, int B, int T, int Cin, int Cout, int k, int Tout) {
  FtGemmBatch b = zero_batch();
  conv_fwd_task(b.t[0], ldx, B, T, Cin, Cout, k, Tout);
  return b;
}
// ft_conv_bank_fwd: K members of 1..K taps as K tasks, most taps first
static FtGemmBatch conv_bank_fwd(int B, int T, int Cin, int C, int K, int Tout) {
  FtGemmBatch b = zero_batch();
  for (int i = 0; i < K; ++i) conv_fwd_task(b.t[K - 1 - i], Cin, B, T, Cin, C, i + 1, Tout);
  return b;
}
// conv1d_bwd_data_impl with transposed tap-major weights
static FtGemmBatch conv_bwd_data(long lddy, int B, int T, int Cin, int Cout, int k, int Tbuf, bool masked) {
  FtGemmBatch b = zero_batch();
  if (masked) b.relu_mask = addr(1);
  FtGemmTask& t = b.t[0];
  t.A = addr(); t.B = addr(); t.C = addr(1);
  t.lda = lddy; t.ldb = Cout; t.ldc = Cin + 9; t.b_tap_stride = (long)Cout * Cin;
  t.M = B * T; t.N = Cin; t.K = Cout; t.taps = k;
  FtRowMap m = {T > 0 ? T : 1, Tbuf, 1, Tbuf, k / 2, -1};
  t.amap = m;
  return b;
}
// ft_conv_bank_bwd_data with transposed weights: chained with scratch (split-K), or the K members as independent tasks
static FtGemmBatch conv_bank_bwd_data(long lddy, int B, int T, int Cin, int C, int K, int Tbuf, bool chained_with_slab) {
  FtGemmBatch b = zero_batch();
  for (int i = 0; i < K; ++i) {
    const int k = i + 1;
    FtGemmTask& t = b.t[i];
    t.A = addr() + (long)i * C; t.B = addr(); t.C = addr(chained_with_slab ? 1 : 0);
    t.lda = lddy; t.ldb = C; t.ldc = Cin; t.b_tap_stride = (long)C * Cin;
    t.M = B * T; t.N = Cin; t.K = C; t.taps = k;
    const int Tvalid = (k % 2 == 0) ? Tbuf : T;
    FtRowMap m = {T > 0 ? T : 1, Tbuf, 1, Tvalid < Tbuf ? Tvalid : Tbuf, k / 2, -1};
    t.amap = m;
  }
  b.chain = chained_with_slab ? K : 0;
  if (chained_with_slab) b.ksplit_slab = addr();
  return b;
}

static FtGemmTNTask zero_tn() {
  FtGemmTNTask t;
  memset(&t, 0, sizeof(t));
  return t;
}
// linear_bw_task: dw [out_f, in_f] = dy^T x over `rows` rows; (B, T, shift): both operands time-major, x read shifted
static FtGemmTNTask linear_tn(int rows, int in_f, int out_f, long lddy, long ldx, int B = 0, int T = 0, int shift = 0) {
  FtGemmTNTask t = zero_tn();
  t.A = addr(); t.B = addr(); t.dst = addr();
  t.lda = lddy; t.ldb = ldx;
  t.ldm = in_f; t.ldn = 1; t.ldj = 0;
  t.M = out_f; t.N = in_f; t.R = rows; t.taps = 1;
  if (B == 0) {
    t.amap = ft_rowmap_identity(rows);
    t.bmap = ft_rowmap_identity(rows);
  } else {
    FtRowMap am = {T, 1, B, T, 0, 0};
    FtRowMap bm = {T, 1, B, T, shift, 0};
    t.amap = am;
    t.bmap = bm;
  }
  return t;
}
// bgemm_tn_task with rows_padded
static FtGemmTNTask bgemm_tn(int M, int N, int R, long lda, long ldb, int rows_padded) {
  FtGemmTNTask t = linear_tn(R, N, M, lda, ldb);
  t.ldm = N + 9;
  t.rowpad = rows_padded;
  t.nz = t.nz1 = 1;
  return t;
}
// conv_bw_task: weight gradient of a k-tap convolution
static FtGemmTNTask conv_tn(int B, int T, int Cin, int Cout, int k) {
  FtGemmTNTask t = zero_tn();
  t.A = addr(); t.B = addr(); t.dst = addr();
  t.lda = Cout; t.ldb = Cin;
  t.ldm = (long)Cin * k; t.ldn = k; t.ldj = 1;
  t.M = Cout; t.N = Cin; t.R = B * T; t.taps = k;
  FtRowMap am = {T, T, 1, T, 0, 0};
  FtRowMap bm = {T, T, 1, T, -(k / 2), 1};
  t.amap = am;
  t.bmap = bm;
  return t;
}
// bank_bw_task: the weight gradients of all K members of a conv bank in one launch
static FtGemmTNTask bank_tn(int B, int T, int Cin, int C, int K, int Tbuf) {
  FtGemmTNTask t = zero_tn();
  t.A = addr(); t.B = addr();
  t.lda = (long)K * C; t.ldb = Cin;
  t.M = K * C; t.N = Cin; t.R = B * Tbuf; t.taps = K;
  FtRowMap am = {Tbuf, Tbuf, 1, Tbuf, 0, 0};
  FtRowMap bm = {Tbuf, T, 1, T, 0, 1};
  t.amap = am;
  t.bmap = bm;
  t.bankC = C;
  t.bankTodd = T;
  return t;
}

// ---- expectations -----------------------------------------------------------------------------------------------------
static void expect_rows(int line, FtGemmBatch b, int ntasks, bool b_ncontig, int precision, const Switches& sw, int variant,
                        int ksplit, int gx, int gy, int gz, long slots = 512) {
  normalise(b, ntasks);
  const RowsPlan p = plan_rows(b, ntasks, b_ncontig, precision, slots, sw);
  const bool big = variant >= FT_GV_ROWS_F32_128_NT_FAST && variant != FT_GV_ROWS_B3_64;
  const bool b3 = variant >= FT_GV_ROWS_B3_64;
  const bool ok = p.variant == variant && p.ksplit == ksplit && p.grid[0] == gx && p.grid[1] == gy && p.grid[2] == gz &&
                  p.big == big && p.b3 == b3 && p.ksplit_floats == (size_t)ksplit * b.t[0].M * b.t[0].N &&
                  p.stat_fused == (b3 && big && b.chain == 0);
  if (!ok) {
    fprintf(stderr, "line %d: rows plan is variant %d ksplit %d grid %d x %d x %d big %d b3 %d fast %d, the table has %d, %d, %d x %d x %d\n",
            line, p.variant, p.ksplit, p.grid[0], p.grid[1], p.grid[2], p.big, p.b3, p.fast, variant, ksplit, gx, gy, gz);
    ++g_failed;
  }
}
#define ROWS(...) expect_rows(__LINE__, __VA_ARGS__)

static void expect_tn(int line, FtGemmTNTask t, int precision, const Switches& sw, int variant, int S, int rps, int gx,
                      int gy, int gz, long slots = 512) {
  normalise(t);
  const TnPlan p = plan_tn(t, precision, slots, sw);
  const int tm = (variant == FT_GV_TN_F32_128_FAST || variant == FT_GV_TN_F32_128_SLOW || variant == FT_GV_TN_B3_128 ||
                  variant == FT_GV_TN_B3P) ? 2 : 1;
  const bool ok = p.variant == variant && p.tm == tm && p.S == S && p.rows_per_split == rps && p.grid[0] == gx &&
                  p.grid[1] == gy && p.grid[2] == gz && p.pipelined == (variant == FT_GV_TN_B3P) &&
                  p.b3 == (variant >= FT_GV_TN_B3_64) && p.need_floats == (size_t)S * t.taps * t.M * t.N &&
                  p.reduce == (t.bankC > 0 ? TN_REDUCE_BANK : t.taps * S <= 16 ? TN_REDUCE_PLAIN : TN_REDUCE_TAP);
  if (!ok) {
    fprintf(stderr, "line %d: TN plan is variant %d tm %d S %d rps %d grid %d x %d x %d, the table has %d, %d, %d, %d, %d x %d x %d\n",
            line, p.variant, p.tm, p.S, p.rows_per_split, p.grid[0], p.grid[1], p.grid[2], variant, tm, S, rps, gx, gy, gz);
    ++g_failed;
  }
}
#define TN(...) expect_tn(__LINE__, __VA_ARGS__)

// ---- the table: rows launches ----------------------------------------------------------------------------------------
static void test_rows_table() {
  const Switches sw = defaults();
  // test_nt_pipelined_k_tails: 12300 rows = 97 row tiles of 128, 130 / 200 columns = 2 column tiles: 194 >= 192 tiles
  for (int N : {130, 200})
    for (int K : {12, 16, 36, 40, 44, 260}) ROWS(linear_fwd(12300, K, N, K + 12), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
  for (int K : {12, 44, 260}) ROWS(linear_fwd(12300, K, 130, K + 12), 1, false, 1, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);     // bf16 mode
  // test_nt_pipelined_time_major_maps (and the bf16 mode of it): 24 x 513 = 12312 rows
  for (int precision : {0, 1}) {
    ROWS(linear_fwd(12312, 36, 200, 40, 24, 0), 1, false, precision, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
    ROWS(linear_fwd(12312, 36, 200, 40, 0, 24), 1, false, precision, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
    ROWS(linear_fwd(12312, 36, 200, 40, 24, 24), 1, false, precision, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
  }
  // test_two_barrier_nt_kernel_behind_a_long_row_stride: a tile's rows span more than 2 GiB
  ROWS(linear_fwd(12312, 36, 200, 34900, 24, 0), 1, false, 0, sw, FT_GV_ROWS_B3_128, 0, 97, 2, 1);
  // test_big_tile_f32_fallback_nt: K % 4 != 0, or the base one float off
  ROWS(linear_fwd(12300, 37, 200, 44), 1, false, 0, sw, FT_GV_ROWS_F32_128_NT_SLOW, 0, 97, 2, 1);
  ROWS(linear_fwd(12300, 37, 130, 44), 1, false, 0, sw, FT_GV_ROWS_F32_128_NT_SLOW, 0, 97, 2, 1);
  ROWS(linear_fwd(12300, 36, 200, 44, 0, 0, 1), 1, false, 0, sw, FT_GV_ROWS_F32_128_NT_SLOW, 0, 97, 2, 1);
  // test_big_tile_f32_nn: ft_linear_bwd_data with an untransposed weight [K = out_f][N = in_f], and ft_bgemm_nn's padded rows
  ROWS(data_multi(1, 12300, 200, 37, 41, false, false), 1, true, 0, sw, FT_GV_ROWS_F32_128_NN_SLOW, 0, 97, 2, 1);
  ROWS(data_multi(1, 12300, 200, 36, 40, false, false), 1, true, 0, sw, FT_GV_ROWS_F32_128_NN_FAST, 0, 97, 2, 1);
  ROWS(bgemm_nn(12300, 200, 37, 40, 1), 1, true, 0, sw, FT_GV_ROWS_F32_128_NN_FAST, 0, 97, 2, 1);
  ROWS(bgemm_nn(12300, 200, 37, 40, 0), 1, true, 0, sw, FT_GV_ROWS_F32_128_NN_SLOW, 0, 97, 2, 1);
  // test_bf16_mode_small_shapes_take_the_64_tile_split_kernels: 333 x 132 = 6 x 3 tiles of 64
  ROWS(linear_fwd(333, 36, 132, 40), 1, false, 1, sw, FT_GV_ROWS_B3_64, 0, 6, 3, 1);
  ROWS(linear_fwd(333, 36, 132, 40), 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 6, 3, 1);
  // test_nt_pipelined_conv_taps_with_k_tail / _conv_data_gradient: 24 x 513 (k = 5) or 24 x 514 (k = 4) rows
  ROWS(conv_fwd(40, 24, 513, 36, 200, 5, 513), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
  ROWS(conv_fwd(40, 24, 513, 36, 200, 4, 514), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
  ROWS(conv_bwd_data(44, 24, 513, 200, 36, 5, 513, true), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
  ROWS(conv_bwd_data(44, 24, 513, 200, 36, 4, 514, false), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
  // test_split_k_of_a_chained_data_gradient: 2 x 129 stages in 8 ranges; without scratch the 64-tile f32 kernel
  for (int rows : {200, 4096})
    for (int tmB : {0, 8}) {
      ROWS(data_multi(2, rows, 132, 2052, 2056, true, true, tmB), 2, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 8, cdiv(rows, 128), 2, 8);
      ROWS(data_multi(2, rows, 132, 2052, 2056, true, false, tmB), 2, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, cdiv(rows, 64), 3, 1);
    }
  // test_split_k_of_the_conv_bank_data_gradient: 9 x 171 = 1539 rows; C = 100: 7 ranges, C = 132: 10 ranges (which the
  // caller's scratch does not hold, so the members run as 8 tasks: 13 x 2 x 8 = 208 tiles)
  ROWS(conv_bank_bwd_data(804, 9, 171, 132, 100, 8, 172, true), 8, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 7, 13, 2, 7);
  ROWS(conv_bank_bwd_data(1060, 9, 171, 132, 132, 8, 172, true), 8, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 10, 13, 2, 10);
  ROWS(conv_bank_bwd_data(1060, 9, 171, 132, 132, 8, 172, false), 8, false, 0, sw, FT_GV_ROWS_B3P, 0, 13, 2, 8);
  // test_linear_fwd_bwd_shapes_land_on_the_64_tile: forward, data gradient (through w^T where out_f % 4 == 0)
  ROWS(linear_fwd(130, 257, 66, 257), 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_SLOW, 0, 3, 2, 1);
  ROWS(data_multi(1, 130, 257, 66, 66, false, false), 1, true, 0, sw, FT_GV_ROWS_F32_64_NN_SLOW, 0, 3, 5, 1);
  ROWS(linear_fwd(333, 10, 7, 10), 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_SLOW, 0, 6, 1, 1);
  ROWS(data_multi(1, 333, 10, 7, 7, false, false), 1, true, 0, sw, FT_GV_ROWS_F32_64_NN_SLOW, 0, 6, 1, 1);
  ROWS(linear_fwd(4096, 256, 512, 256), 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 8, 1);
  ROWS(data_multi(1, 4096, 256, 512, 512, true, false), 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 4, 1);
  // split counts of ft_linear_bwd_data_multi_workspace(n, rows, in_f, out_f) / (4 rows in_f), 512 slots
  ROWS(data_multi(2, 4096, 512, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 4, 32, 4, 4);
  ROWS(data_multi(1, 4096, 512, 2048, 2048, true, true), 1, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 4, 32, 4, 4);
  ROWS(data_multi(2, 128, 512, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 8, 1, 4, 8);
  ROWS(data_multi(2, 4100, 100, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 8, 33, 1, 8);
  ROWS(data_multi(2, 4100, 132, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 7, 33, 2, 7);
  ROWS(data_multi(2, 128, 512, 8192, 8192, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 16, 1, 4, 16);         // the cap
  ROWS(data_multi(1, 256, 256, 16384, 16384, true, true), 1, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 16, 2, 2, 16);
  ROWS(data_multi(2, 4096, 256, 768, 768, true, true), 2, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 4, 1);      // 96 stages < 128
  ROWS(data_multi(2, 26912, 512, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P, 0, 211, 4, 1);             // 844 tiles > 256
  // the benchmark's dominant launch (bench.py BANK_SHAPE): the postnet conv bank forward, 32 x 842 rows, 80 -> 256, 8
  // members of 1..8 taps as 8 tasks of one pipelined launch
  ROWS(conv_bank_fwd(32, 841, 80, 256, 8, 842), 8, false, 0, sw, FT_GV_ROWS_B3P, 0, 211, 2, 8);
  // a CU-limited stream's 128 slots: 32 x 4 tiles leave room for one range only
  ROWS(data_multi(2, 4096, 512, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 8, 1, 128);
  // the scratch query's answer, from the un-normalised batch as ft_rows_ksplit_floats passes it
  CHECK(rows_ksplit_floats(data_multi(2, 4096, 512, 2048, 2048, true, false), 2, 512, sw) == 4u * 4096 * 512);
  CHECK(rows_ksplit_floats(data_multi(2, 4096, 256, 768, 768, true, false), 2, 512, sw) == 0);
}

// ---- the table: TN launches ------------------------------------------------------------------------------------------
static void test_tn_table() {
  const Switches sw = defaults();
  // TN_SHAPES (out_f, in_f, rows) with test_tn_big_tile_tails' leading dimensions
  TN(linear_tn(9001, 516, 1000, 1008, 520), 0, sw, FT_GV_TN_B3P, 12, 768, 8, 5, 12);
  // aligned: 8 x 9 = 72 tiles of 128 into 512 slots, rounded DOWN: 7 (the query's 8 is the unaligned plan's, rounded up)
  TN(linear_tn(2001, 1100, 1000, 1008, 1104), 0, sw, FT_GV_TN_B3_128, 7, 288, 8, 9, 7);
  // out_f or in_f % 4 != 0: 16 x 9 = 144 tiles of 64 -> 512 / 144 rounded up = 4 (the query's 12 is the aligned plan's)
  TN(linear_tn(9001, 516, 1001, 1008, 520), 0, sw, FT_GV_TN_F32_64_SLOW, 4, 2272, 16, 9, 4);
  TN(linear_tn(9001, 518, 1000, 1008, 524), 0, sw, FT_GV_TN_F32_64_SLOW, 4, 2272, 16, 9, 4);
  TN(linear_tn(2001, 1100, 1001, 1008, 1104), 0, sw, FT_GV_TN_F32_128_SLOW, 8, 256, 8, 9, 8);
  // test_tn_big_tile_padded_rows (ft_bgemm_tn, rows_padded)
  TN(bgemm_tn(1001, 518, 9001, 1004, 520, 1), 0, sw, FT_GV_TN_B3P, 12, 768, 8, 5, 12);
  TN(bgemm_tn(1001, 1102, 2001, 1004, 1104, 1), 0, sw, FT_GV_TN_B3_128, 7, 288, 8, 9, 7);
  // test_tn_big_tile_time_major_shift: 17 x 529 = 8993 and 4 x 501 = 2004 rows
  for (int shift : {1, -1}) {
    TN(linear_tn(8993, 516, 1000, 1004, 524, 17, 529, shift), 0, sw, FT_GV_TN_B3P, 12, 768, 8, 5, 12);
    TN(linear_tn(2004, 1100, 1000, 1004, 1108, 4, 501, shift), 0, sw, FT_GV_TN_B3_128, 7, 288, 8, 9, 7);
  }
  // test_bf16_mode_small_shapes_take_the_64_tile_split_kernels: 3 x 1 tiles of 64, at least 128 rows per split: S = 3
  TN(linear_tn(333, 36, 132, 136, 40), 1, sw, FT_GV_TN_B3_64, 3, 128, 3, 1, 3);
  // test_linear_fwd_bwd_shapes_land_on_the_64_tile
  TN(linear_tn(130, 257, 66, 66, 257), 0, sw, FT_GV_TN_F32_64_SLOW, 2, 96, 2, 5, 2);
  TN(linear_tn(333, 10, 7, 7, 10), 0, sw, FT_GV_TN_F32_64_SLOW, 3, 128, 1, 1, 3);
  TN(linear_tn(4096, 256, 512, 512, 256), 0, sw, FT_GV_TN_F32_64_FAST, 16, 256, 8, 4, 16);
  // split counts of ft_linear_bwd_weight_workspace(rows, in_f, out_f) / (4 in_f out_f), 512 slots
  TN(linear_tn(26912, 256, 256, 256, 256), 0, sw, FT_GV_TN_F32_64_FAST, 32, 864, 4, 4, 32);
  TN(linear_tn(4096, 512, 2048, 2048, 512), 0, sw, FT_GV_TN_B3P, 8, 512, 16, 4, 8);
  TN(linear_tn(100, 80, 80, 80, 80), 0, sw, FT_GV_TN_F32_64_FAST, 1, 128, 2, 2, 1);
  TN(linear_tn(26912, 80, 256, 256, 80), 0, sw, FT_GV_TN_F32_64_FAST, 61, 448, 4, 2, 61);
  // at the edges of the tile rule: exactly 64 tiles of 128 take the 128 tile whatever the alignment (the GPU suite: "64
  // tile below 64 tiles of 128"); 40 tiles x (5000 / 1024 = 4) = 160 < 256 stays on the 64 tile, 4 splits either way;
  // out_f = 128 with 64 tiles is big (8 splits), out_f = 64 never is (4 splits)
  TN(linear_tn(200, 1022, 1021, 1024, 1024), 0, sw, FT_GV_TN_F32_128_SLOW, 2, 128, 8, 8, 2);
  TN(linear_tn(5000, 516, 1000, 1000, 516), 0, sw, FT_GV_TN_F32_64_FAST, 4, 1280, 16, 9, 4);
  TN(linear_tn(2000, 8192, 128, 128, 8192), 0, sw, FT_GV_TN_B3_128, 8, 256, 1, 64, 8);
  TN(linear_tn(4096, 8192, 64, 64, 8192), 0, sw, FT_GV_TN_F32_64_FAST, 4, 1024, 1, 128, 4);
  // the benchmark's largest weight gradient (bench.py wgrad_family): the decoder LSTM's W_ih, 2048 x 512 over 26912
  // time-major rows of a [T, B, 4096] gradient
  {
    FtGemmTNTask t = linear_tn(26912, 512, 2048, 4096, 512, 32, 841, 0);
    const FtRowMap batch_major = {841, 841, 1, 841, 0, 0};
    t.bmap = batch_major;
    TN(t, 0, sw, FT_GV_TN_B3P, 8, 3392, 16, 4, 8);
  }
  // the postnet conv bank's weight gradient (ft_conv_bank_bwd_weight_workspace(32, 841, 80, 256, 8, 842): 29 slabs):
  // 256 / 128 x 36 live (member, tap) pairs along x
  TN(bank_tn(32, 841, 80, 256, 8, 842), 0, sw, FT_GV_TN_B3P, 29, 960, 72, 1, 29);
  // a 5-tap convolution's weight gradient: 4 x 4 x 5 = 80 tiles into 512 slots, rounded DOWN: 6 (the query,
  // ft_conv1d_bwd_weight_workspace(32, 841, 512, 512, 5, 841), answers the unaligned plan's 7)
  TN(conv_tn(32, 841, 512, 512, 5), 0, sw, FT_GV_TN_B3P, 6, 4512, 4, 4, 30);
}

// ---- every switch's other side ---------------------------------------------------------------------------------------
static void test_switches() {
  const Switches d = defaults();
  CHECK(d.b3 == 1 && d.b3_tn == 1 && d.ksplit == 1 && d.pipe == 1 && d.tn_pipe == 1 && d.tn_force_s == 0 && d.log == 0);
  CHECK(with("FT_GEMM_B3_TN", "0").b3_tn == 0 && with("FT_GEMM_B3_TN", "1").b3_tn == 2 && with("FT_GEMM_B3_TN", "x").b3_tn == 1);
  CHECK(with("FT_GEMM_B3", "0").b3 == 0 && with("FT_GEMM_B3", "1").b3 == 1 && with("FT_GEMM_B3", "").b3 == 1);
  CHECK(with("FT_GEMM_LOG", "1").log == 1 && with("FT_GEMM_LOG", "0").log == 0 && with("FT_GEMM_LOG", "2").log == 0);
  CHECK(with("FT_TN_FORCE_S", "3").tn_force_s == 3 && with("FT_GEMM_KSPLIT", "0").ksplit == 0);
  CHECK(with("FT_GEMM_PIPE", "0").pipe == 0 && with("FT_GEMM_TN_PIPE", "0").tn_pipe == 0);
  CHECK(with("FT_GEMM_B3", "0").tn_b3_mode() == 0 && with("FT_GEMM_B3_TN", "1").tn_b3_mode() == 2);
  // FT_GEMM_B3=0: the f32 kernels, rows and TN, and no split-K (only the pipelined bf16-pipe kernel has it)
  ROWS(linear_fwd(12300, 36, 200, 48), 1, false, 0, with("FT_GEMM_B3", "0"), FT_GV_ROWS_F32_128_NT_FAST, 0, 97, 2, 1);
  ROWS(data_multi(2, 4096, 132, 2052, 2056, true, true), 2, false, 0, with("FT_GEMM_B3", "0"), FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 3, 1);
  // (without the split path's preference 40 tiles of 128 are "small": the unaligned plan of the table above)
  TN(linear_tn(9001, 516, 1000, 1008, 520), 0, with("FT_GEMM_B3", "0"), FT_GV_TN_F32_64_FAST, 4, 2272, 16, 9, 4);
  // ... but the bf16 precision mode still takes the bf16 pipe
  ROWS(linear_fwd(12300, 36, 200, 48), 1, false, 1, with("FT_GEMM_B3", "0"), FT_GV_ROWS_B3P, 0, 97, 2, 1);
  // FT_GEMM_PIPE=0: the two-barrier rows kernel, which cannot split K
  ROWS(linear_fwd(12300, 36, 200, 48), 1, false, 0, with("FT_GEMM_PIPE", "0"), FT_GV_ROWS_B3_128, 0, 97, 2, 1);
  ROWS(data_multi(2, 4096, 132, 2052, 2056, true, true), 2, false, 0, with("FT_GEMM_PIPE", "0"), FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 3, 1);
  // FT_GEMM_KSPLIT=0: scratch offered, not split
  ROWS(data_multi(2, 4096, 132, 2052, 2056, true, true), 2, false, 0, with("FT_GEMM_KSPLIT", "0"), FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 3, 1);
  // FT_GEMM_TN_PIPE=0: the two-barrier TN kernel, same split
  TN(linear_tn(9001, 516, 1000, 1008, 520), 0, with("FT_GEMM_TN_PIPE", "0"), FT_GV_TN_B3_128, 12, 768, 8, 5, 12);
  // FT_GEMM_B3_TN=0: f32 TN kernels (and the unaligned plan's tile and split); =1: the 64 tile takes the bf16 pipe too
  TN(linear_tn(9001, 516, 1000, 1008, 520), 0, with("FT_GEMM_B3_TN", "0"), FT_GV_TN_F32_64_FAST, 4, 2272, 16, 9, 4);
  TN(linear_tn(4096, 256, 512, 512, 256), 0, with("FT_GEMM_B3_TN", "1"), FT_GV_TN_B3_64, 16, 256, 8, 4, 16);
  // FT_TN_FORCE_S=3: three splits of 9001 / 3 = 3001 -> 3008 rows
  TN(linear_tn(9001, 516, 1000, 1008, 520), 0, with("FT_TN_FORCE_S", "3"), FT_GV_TN_B3P, 3, 3008, 8, 5, 3);
}

// ---- both sides of every threshold --------------------------------------------------------------------------------------
// Rows that sit on a threshold of the header and one step beside it.  Their values are the launchers' own before the
// planner moved into the header (recorded from that code; the split counts are also what the workspace queries answered,
// tests/test_gemm_plan_cpu.py), so a threshold that drifts by one fails a row here.
static FtGemmBatch with_map(FtGemmBatch b, FtRowMap m) {
  b.t[0].amap = m;
  return b;
}
static FtGemmBatch with_ld(FtGemmBatch b, long lda, long ldb) {
  for (int i = 0; i < FT_MAX_TASKS; ++i) {
    b.t[i].lda = lda;
    b.t[i].ldb = ldb;
  }
  return b;
}
static FtGemmBatch with_nz(FtGemmBatch b, int nz, long sA0) {
  FtGemmTask& t = b.t[0];
  t.nz = nz;
  t.nz1 = 1;
  t.sA0 = sA0;
  t.sA1 = t.sB0 = t.sB1 = 10804;
  return b;
}
static FtGemmTNTask tn_maps(FtGemmTNTask t, FtRowMap am, FtRowMap bm) {
  t.amap = am;
  t.bmap = bm;
  return t;
}

static void test_rows_boundaries() {
  const Switches sw = defaults();
  // the 128 tile: 192 tiles of 128 (96 x 2; chained: per product), more than 64 rows and columns, strided instances count
  ROWS(linear_fwd(12288, 36, 200, 40), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 96, 2, 1);
  ROWS(linear_fwd(12160, 36, 200, 40), 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 190, 4, 1);
  ROWS(linear_fwd(65, 36, 24576, 40), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 1, 192, 1);
  ROWS(linear_fwd(64, 36, 24576, 40), 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 1, 384, 1);
  ROWS(linear_fwd(24576, 36, 65, 40), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 192, 1, 1);
  ROWS(linear_fwd(24576, 36, 64, 40), 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 384, 1, 1);
  ROWS(data_multi(2, 12288, 200, 36, 40, true, false), 2, false, 0, sw, FT_GV_ROWS_B3P, 0, 96, 2, 1);
  ROWS(data_multi(2, 12160, 200, 36, 40, true, false), 2, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 190, 4, 1);
  ROWS(with_nz(bgemm_nn(300, 200, 36, 36, 0), 32, 10804), 1, true, 0, sw, FT_GV_ROWS_F32_128_NN_FAST, 0, 3, 2, 32);
  ROWS(with_nz(bgemm_nn(300, 200, 36, 36, 0), 31, 10804), 1, true, 0, sw, FT_GV_ROWS_F32_64_NN_FAST, 0, 5, 4, 31);
  {
    FtGemmBatch b = linear_fwd(333, 36, 132, 40);
    b.force_tile = 2;
    ROWS(b, 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 3, 2, 1);
    b = linear_fwd(12300, 36, 200, 40);
    b.force_tile = 1;
    ROWS(b, 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 193, 4, 1);
  }
  // 16-byte loads: every term of the alignment predicate, N % 4 of the NN form
  ROWS(linear_fwd(12300, 36, 200, 41), 1, false, 0, sw, FT_GV_ROWS_F32_128_NT_SLOW, 0, 97, 2, 1);
  ROWS(with_nz(bgemm_nn(300, 200, 36, 36, 0), 32, 10806), 1, true, 0, sw, FT_GV_ROWS_F32_128_NN_SLOW, 0, 3, 2, 32);
  ROWS(bgemm_nn(12300, 202, 36, 36, 0), 1, true, 0, sw, FT_GV_ROWS_F32_128_NN_SLOW, 0, 97, 2, 1);
  {
    FtGemmBatch b = conv_fwd(40, 24, 513, 36, 200, 5, 513);
    b.t[0].b_tap_stride += 2;
    ROWS(b, 1, false, 0, sw, FT_GV_ROWS_F32_128_NT_SLOW, 0, 97, 2, 1);
    b = with_nz(bgemm_nn(300, 200, 36, 36, 0), 32, 10804);
    b.t[0].sB1 = 2;
    ROWS(b, 1, true, 0, sw, FT_GV_ROWS_F32_128_NN_SLOW, 0, 3, 2, 32);
    b = with_nz(bgemm_nn(300, 200, 36, 36, 0), 32, 10804);
    b.t[0].sA1 = 2;
    ROWS(b, 1, true, 0, sw, FT_GV_ROWS_F32_128_NN_SLOW, 0, 3, 2, 32);
    b = with_nz(bgemm_nn(300, 200, 36, 36, 0), 32, 10804);
    b.t[0].sB0 = 2;
    ROWS(b, 1, true, 0, sw, FT_GV_ROWS_F32_128_NN_SLOW, 0, 3, 2, 32);
    b = conv_fwd(40, 24, 513, 36, 200, 5, 513);
    b.t[0].b_tap_stride = 7204;
    ROWS(b, 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
  }
  // 190 tiles of 128 that 127-wide tiles would count as 285
  ROWS(linear_fwd(12160, 36, 256, 40), 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 190, 4, 1);
  {
  }
  // the pipelined kernel's 31-bit offsets: 12428 rows of a tile's span x lda x 4 and 128 x ldb x 4 below 2^31, no negative
  // stride; a batch-major map of 16-row items spans 128 / 16 + 2 items
  ROWS(linear_fwd(12300, 36, 200, 43196), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
  ROWS(linear_fwd(12300, 36, 200, 43200), 1, false, 0, sw, FT_GV_ROWS_B3_128, 0, 97, 2, 1);
  ROWS(with_ld(linear_fwd(12300, 36, 200, 40), 40, 4194300), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 97, 2, 1);
  ROWS(with_ld(linear_fwd(12300, 36, 200, 40), 40, 4194304), 1, false, 0, sw, FT_GV_ROWS_B3_128, 0, 97, 2, 1);
  ROWS(with_map(linear_fwd(12288, 36, 200, 40), FtRowMap{16, 1342174, 1, 16, 0, 0}), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 96, 2, 1);
  ROWS(with_map(linear_fwd(12288, 36, 200, 40), FtRowMap{16, 1342175, 1, 16, 0, 0}), 1, false, 0, sw, FT_GV_ROWS_B3_128, 0, 96, 2, 1);
  ROWS(with_map(linear_fwd(12288, 36, 200, 40), FtRowMap{16, 16, -1, 16, 0, 0}), 1, false, 0, sw, FT_GV_ROWS_B3_128, 0, 96, 2, 1);
  {                                                  // every task of a launch is held to the bound
    FtGemmBatch b = conv_bank_fwd(32, 841, 80, 256, 8, 842);
    b.t[5].lda = 43200;
    ROWS(b, 8, false, 0, sw, FT_GV_ROWS_B3P, 0, 211, 2, 8);
  }
  ROWS(with_map(linear_fwd(12288, 36, 200, 40), FtRowMap{16, 16, 0, 16, 0, 0}), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 96, 2, 1);
  // (896 + 128) rows x 2^19 floats x 4 is 2^31 exactly: refused
  ROWS(linear_fwd(896, 36, 3584, 524288), 1, false, 0, sw, FT_GV_ROWS_B3_128, 0, 7, 28, 1);
  ROWS(linear_fwd(896, 36, 3584, 524284), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 7, 28, 1);
  ROWS(with_map(linear_fwd(12288, 36, 200, 40), FtRowMap{16, -16, 1, 16, 0, 0}), 1, false, 0, sw, FT_GV_ROWS_B3_128, 0, 96, 2, 1);
  // split-K: 128 stages of 16 (K = 2033..2048) but not 127; more than 64 rows and columns; N % 4; 2 ranges but not 1
  // (256 / 260 tiles into 512 slots); K % 4 of every task; fp32 and NT only; a plain epilogue only
  ROWS(data_multi(1, 4096, 512, 2032, 2032, true, true), 1, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 8, 1);
  ROWS(data_multi(1, 4096, 512, 2036, 2036, true, true), 1, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 4, 32, 4, 4);
  ROWS(data_multi(2, 65, 512, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 8, 1, 4, 8);
  ROWS(data_multi(2, 64, 512, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 1, 8, 1);
  ROWS(data_multi(2, 4096, 68, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 8, 32, 1, 8);
  ROWS(data_multi(2, 4096, 64, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 1, 1);
  ROWS(data_multi(2, 4096, 510, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 8, 1);
  ROWS(data_multi(2, 8192, 512, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 2, 64, 4, 2);
  ROWS(data_multi(2, 8256, 512, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P, 0, 65, 4, 1);
  ROWS(data_multi(2, 4096, 516, 2048, 2048, true, true), 2, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 3, 32, 5, 3);
  ROWS(data_multi(1, 128, 512, 4112, 4112, true, true), 1, false, 0, sw, FT_GV_ROWS_B3P_KSPLIT, 8, 1, 4, 8);
  ROWS(with_ld(data_multi(2, 4096, 512, 2050, 2052, true, true), 2052, 2052), 2, false, 0, sw, FT_GV_ROWS_F32_64_NT_SLOW, 0, 64, 8, 1);
  ROWS(data_multi(2, 4096, 512, 2048, 2048, true, true), 2, false, 1, sw, FT_GV_ROWS_B3_64, 0, 64, 8, 1);
  ROWS(data_multi(2, 4096, 512, 2048, 2048, false, true), 2, true, 0, sw, FT_GV_ROWS_F32_64_NN_FAST, 0, 64, 8, 1);
  for (int what = 0; what < 6; ++what) {
    FtGemmBatch b = data_multi(2, 4096, 512, 2048, 2048, true, true);
    if (what == 0) b.t[0].relu = 1;
    if (what == 1) b.t[0].scale = addr();
    if (what == 2) b.t[0].stat = reinterpret_cast<double*>(addr());
    if (what == 3) b.hw_mode = 2;
    if (what == 4) b.relu_mask = addr();
    if (what == 5) b.out_lens = reinterpret_cast<const long*>(addr());
    ROWS(b, 2, false, 0, sw, FT_GV_ROWS_F32_64_NT_FAST, 0, 64, 8, 1);
  }
  // (two strided instances: 2 x 128 tiles take the 128 tile, unsplit)
  ROWS(with_nz(data_multi(1, 4096, 512, 2048, 2048, true, true), 2, 0), 1, false, 0, sw, FT_GV_ROWS_B3P, 0, 32, 4, 2);
}

static void test_tn_boundaries() {
  const Switches sw = defaults();
  // the 128 tile of aligned operands below 64 tiles: tiles x (R / 1024) >= 256 (32 x 8, not 32 x 7), more than 64 rows and
  // columns of output
  TN(linear_tn(8192, 1024, 512, 512, 1024), 0, sw, FT_GV_TN_B3P, 16, 512, 4, 8, 16);
  TN(linear_tn(8191, 1024, 512, 512, 1024), 0, sw, FT_GV_TN_F32_64_FAST, 4, 2048, 8, 16, 4);
  TN(bgemm_tn(65, 2048, 16384, 68, 2048, 1), 0, sw, FT_GV_TN_B3P, 32, 512, 1, 16, 32);
  TN(bgemm_tn(64, 2048, 16384, 64, 2048, 1), 0, sw, FT_GV_TN_F32_64_FAST, 16, 1024, 1, 32, 16);
  TN(bgemm_tn(2048, 65, 16384, 2048, 68, 1), 0, sw, FT_GV_TN_B3P, 32, 512, 16, 1, 32);
  TN(bgemm_tn(2048, 64, 16384, 2048, 64, 1), 0, sw, FT_GV_TN_F32_64_FAST, 16, 1024, 32, 1, 16);
  TN(linear_tn(8191, 512, 1024, 1024, 512), 0, sw, FT_GV_TN_F32_64_FAST, 4, 2048, 16, 8, 4);
  TN(linear_tn(7168, 1024, 516, 516, 1024), 0, sw, FT_GV_TN_B3P, 12, 608, 5, 8, 12);
  TN(linear_tn(7168, 516, 1024, 1024, 516), 0, sw, FT_GV_TN_B3P, 12, 608, 8, 5, 12);
  TN(linear_tn(5120, 2176, 384, 384, 2176), 0, sw, FT_GV_TN_F32_64_FAST, 3, 1728, 6, 34, 3);                  // 51 tiles x 5 = 255
  // unaligned operands: 63 tiles are few, 64 are not; 64 rows or columns of output are few, 65 are not
  TN(linear_tn(200, 1150, 895, 896, 1152), 0, sw, FT_GV_TN_F32_64_SLOW, 2, 128, 14, 18, 2);
  TN(linear_tn(4096, 64, 8192, 8192, 64), 0, sw, FT_GV_TN_F32_64_FAST, 4, 1024, 128, 1, 4);
  TN(linear_tn(4096, 8192, 65, 68, 8192), 0, sw, FT_GV_TN_F32_128_SLOW, 8, 512, 1, 64, 8);
  TN(linear_tn(4096, 65, 8192, 8192, 68), 0, sw, FT_GV_TN_F32_128_SLOW, 8, 512, 64, 1, 8);
  // splits: 512 slots over 73 tiles rounded up (8), at least 128 rows each (129 rows: 2)
  TN(linear_tn(4096, 4672, 64, 64, 4672), 0, sw, FT_GV_TN_F32_64_FAST, 8, 512, 1, 73, 8);
  TN(linear_tn(129, 80, 80, 80, 80), 0, sw, FT_GV_TN_F32_64_FAST, 2, 96, 2, 2, 2);
  TN(linear_tn(128, 80, 80, 80, 80), 0, sw, FT_GV_TN_F32_64_FAST, 1, 128, 2, 2, 1);
  TN(linear_tn(4096, 4096, 4096, 4096, 4096), 0, sw, FT_GV_TN_B3P, 1, 4096, 32, 32, 1);                // more tiles than slots: one split
  TN(linear_tn(17408, 768, 640, 640, 768), 0, sw, FT_GV_TN_B3P, 17, 1024, 5, 6, 17);                   // 17 slabs: the per-tap reduce
  TN(linear_tn(9001, 516, 1000, 1008, 520), 0, with("FT_TN_FORCE_S", "1"), FT_GV_TN_B3P, 1, 9024, 8, 5, 1);
  TN(linear_tn(2001, 1100, 1000, 1008, 1104), 0, with("FT_GEMM_B3_TN", "0"), FT_GV_TN_F32_128_FAST, 8, 256, 8, 9, 8);
  // padded rows need the leading dimension to hold the padding
  TN(bgemm_tn(1001, 518, 9001, 1000, 520, 1), 0, sw, FT_GV_TN_F32_64_SLOW, 4, 2272, 16, 9, 4);
  TN(bgemm_tn(1001, 518, 9001, 1004, 516, 1), 0, sw, FT_GV_TN_F32_64_SLOW, 4, 2272, 16, 9, 4);
  // one row: one split of the smallest size
  TN(linear_tn(1, 80, 80, 80, 80), 0, sw, FT_GV_TN_F32_64_FAST, 1, 32, 2, 2, 1);
  // the pipelined kernel: from 512 rows per split (not 480), items of at least 16 rows (not 15) that both maps share
  TN(linear_tn(3840, 512, 2048, 2048, 512), 0, sw, FT_GV_TN_B3_128, 8, 480, 16, 4, 8);
  TN(linear_tn(9008, 516, 1000, 1004, 524, 563, 16, 1), 0, sw, FT_GV_TN_B3P, 12, 768, 8, 5, 12);
  TN(linear_tn(9000, 516, 1000, 1004, 524, 600, 15, 1), 0, sw, FT_GV_TN_B3_128, 12, 768, 8, 5, 12);
  TN(tn_maps(linear_tn(8993, 516, 1000, 1004, 524), ft_rowmap_identity(8993), FtRowMap{529, 529, 1, 529, 0, 0}), 0, sw, FT_GV_TN_B3_128, 12, 768, 8, 5, 12);
  // ... and byte offsets below 2^31 from either operand's base: (rows + 16 + the furthest shift + taps + 1) x ld x 4 + 1024,
  // identity maps (532591 rows fit, 532592 do not), time-major maps read one step later (17 x 500 fit, 17 x 501 do not),
  // 1024 bytes of slack (2^31 - 16 + 1024 does not fit), no negative stride
  TN(linear_tn(532591, 516, 1000, 1008, 1008), 0, sw, FT_GV_TN_B3P, 12, 44384, 8, 5, 12);
  TN(linear_tn(532592, 516, 1000, 1008, 1008), 0, sw, FT_GV_TN_B3_128, 12, 44384, 8, 5, 12);
  TN(linear_tn(532592, 516, 1000, 1004, 1008), 0, sw, FT_GV_TN_B3_128, 12, 44384, 8, 5, 12);
  TN(linear_tn(532592, 516, 1000, 1008, 1004), 0, sw, FT_GV_TN_B3_128, 12, 44384, 8, 5, 12);
  TN(linear_tn(8500, 516, 1000, 60832, 60832, 17, 500, 1), 0, sw, FT_GV_TN_B3P, 12, 736, 8, 5, 12);
  TN(linear_tn(8517, 516, 1000, 60832, 60832, 17, 501, 1), 0, sw, FT_GV_TN_B3_128, 12, 736, 8, 5, 12);
  TN(linear_tn(8501, 516, 1000, 60832, 60832, 17, 500, 1), 0, sw, FT_GV_TN_B3_128, 12, 736, 8, 5, 12);   // a row into an 18th item
  {                                                  // five taps from -2 on: the last tap's shift, 2, counts (853 rows fit, 854 do not)
    FtGemmTNTask c = conv_tn(32, 853, 512, 512, 5);
    c.ldb = 18496;
    TN(c, 0, sw, FT_GV_TN_B3P, 6, 4576, 4, 4, 30);
    c = conv_tn(32, 854, 512, 512, 5);
    c.ldb = 18496;
    TN(c, 0, sw, FT_GV_TN_B3_128, 6, 4576, 4, 4, 30);
  }
  TN(linear_tn(299575, 256, 256, 1792, 1792), 0, sw, FT_GV_TN_B3_128, 127, 2368, 2, 2, 127);                // 2^31 exactly: refused
  TN(linear_tn(1838581, 256, 256, 292, 292), 0, sw, FT_GV_TN_B3_128, 128, 14368, 2, 2, 128);
  TN(linear_tn(1838580, 256, 256, 292, 292), 0, sw, FT_GV_TN_B3P, 128, 14368, 2, 2, 128);
  TN(tn_maps(linear_tn(8993, 516, 1000, 1004, 524), FtRowMap{529, 529, -1, 529, 0, 0}, FtRowMap{529, 529, 1, 529, 0, 0}), 0, sw, FT_GV_TN_B3_128, 12, 768, 8, 5, 12);
  TN(tn_maps(linear_tn(8993, 516, 1000, 1004, 524), FtRowMap{529, 529, 1, 529, 0, 0}, FtRowMap{529, -529, 1, 529, 0, 0}), 0, sw, FT_GV_TN_B3_128, 12, 768, 8, 5, 12);
  // the grid's z limit: 65535 splits of 160 rows fit it exactly (one split fewer would round to 192 rows)
  TN(linear_tn(65535 * 160, 8, 8, 8, 8), 0, with("FT_TN_FORCE_S", "70000"), FT_GV_TN_F32_64_FAST, 65535, 160, 1, 1, 65535);
}

// ---- conditions every plan meets ---------------------------------------------------------------------------------------
static void test_invariants() {
  const Switches sw = defaults();
  const int dims[] = {1, 63, 64, 65, 128, 129, 1000}, depths[] = {1, 15, 16, 127, 4096, 26912};
  long plans = 0;
  for (int M : dims)
    for (int N : dims)
      for (int R : depths)
        for (int taps : {1, 5})
          for (long slots : {128L, 512L}) {
            for (int aligned : {0, 1}) {
              FtGemmTNTask t = conv_tn(1, R, N, M, taps);
              t.rowpad = aligned;
              t.lda = (M + 3) & ~3;
              t.ldb = (N + 3) & ~3;
              normalise(t);
              const TnPlan p = plan_tn(t, 0, slots, sw);
              CHECK(p.fast == (aligned || (M % 4 == 0 && N % 4 == 0)));
              CHECK(p.S >= 1 && p.rows_per_split % 16 == 0);
              CHECK((long)p.S * p.rows_per_split >= R && (long)(p.S - 1) * p.rows_per_split < R);
              CHECK(p.grid[0] >= 1 && p.grid[1] >= 1 && p.grid[1] <= 65535 && p.grid[2] >= 1 && p.grid[2] <= 65535);
              CHECK(p.grid[0] == cdiv(M, 64 * p.tm) && p.grid[1] == cdiv(N, 64 * p.tm) && p.grid[2] == p.S * taps);
              CHECK(p.need_floats == (size_t)p.S * taps * t.nz * M * N);
              CHECK(!p.pipelined || (p.b3 && p.tm == 2 && p.rows_per_split >= 512));
              ++plans;
            }
            // the same shape as a chained data gradient of two tasks with scratch, K = R, and as a tap convolution
            for (int chained : {0, 1}) {
              FtGemmBatch b = chained ? data_multi(2, M, N, R, (R + 3) & ~3, true, true) : conv_fwd((R + 3) & ~3, 1, M, R, N, taps, M);
              if (!chained) b.ksplit_slab = addr();
              const int ntasks = chained ? 2 : 1;
              normalise(b, ntasks);
              const RowsPlan p = plan_rows(b, ntasks, false, 0, slots, sw);
              CHECK(p.grid[0] == cdiv(M, p.big ? 128 : 64) && p.grid[1] == cdiv(N, p.big ? 128 : 64));
              CHECK(p.grid[1] <= 65535 && p.grid[2] >= 1 && p.grid[2] <= 65535);
              CHECK(p.ksplit == 0 || p.ksplit >= 2);
              CHECK(p.ksplit_floats == (size_t)p.ksplit * M * N);
              if (p.ksplit) {                      // a split-K plan is always big and pipelined
                CHECK(p.big && p.b3 && p.fast && p.variant == FT_GV_ROWS_B3P_KSPLIT && p.grid[2] == p.ksplit);
                CHECK((long)p.ksplit * p.grid[0] * p.grid[1] <= slots && p.stat_fused == !chained);
              } else {
                CHECK(p.variant != FT_GV_ROWS_B3P_KSPLIT && p.grid[2] == 1);
              }
              ++plans;
            }
          }
  CHECK(plans == 7 * 7 * 6 * 2 * 2 * 4);
  CHECK(tiles_big(192, 65, 65) && !tiles_big(191, 1000, 1000) && !tiles_big(1000, 64, 1000) && !tiles_big(1000, 1000, 64));
}

int main() {
  test_rows_table();
  test_tn_table();
  test_switches();
  test_rows_boundaries();
  test_tn_boundaries();
  test_invariants();
  if (g_failed) {
    fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("gemm plan: ok\n");
  return 0;
}
