// Stand-alone host test of csrc/ft_reduce_plan.h (tests/test_reduce_plan_cpu.py builds it with the sanitizers and runs it):
// the chunk plan of the column reductions against a hand-written table, and the scratch sizes composed from it -- the
// batched column sums, the convolutions' statistics buffers, the two "independent tasks + ordered sum" choices and the
// three workspaces of an FFTBlock backward -- against the conditions they must meet over a sweep of shapes.
//
// Where the table comes from (never from the header under test): worked out by hand from the rule "about 64 rows per
// chunk at least, at most clamp(1024 / column tiles, 16, 64) chunks, rows per chunk a multiple of 4 and at least 4";
// the chunk counts of the first seven rows are the ones tests/bn_cpu.py pins (BN_CHUNKS) and the GPU tests observe.
#include <stdio.h>

#include <initializer_list>

#include "ft_reduce_plan.h"

using namespace reduce_plan;

static int g_failed = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                               \
    }                                                           \
  } while (0)

static const char* no_env(const char*) { return nullptr; }

static void test_chunk_table() {
  struct Row {
    long rows;
    int C, nchunks, rpc;
  };
  const Row table[] = {
      // tests/bn_cpu.py: BN_CHUNKS, (B, Tbuf, C) -> rows = B * Tbuf
      {5 * 13, 64, 2, 36},       // 2 chunks of ceil(65 / 2) = 33 -> 36 rows
      {1 * 1, 64, 1, 4},         // the floor of 4 rows per chunk
      {3 * 70, 64, 4, 56},       // ceil(210 / 64) = 4 chunks of 53 -> 56
      {7 * 59, 64, 7, 60},       // 413 rows: 7 chunks of 59 -> 60
      {9 * 61, 64, 9, 64},       // 549 rows: 9 chunks of 61 -> 64
      {27 * 161, 64, 64, 68},    // 4347 rows: the cap of 64 chunks, 68 rows each (63 * 68 < 4347)
      {3 * 70, 70, 4, 56},       // two column tiles: 512 wanted, capped at 64; the rows decide
      // want clamped from below at 16: 1024 / 64 tiles is 16 exactly, 1024 / 65 tiles would be 15
      {4096, 4096, 16, 256}, {4096, 4097, 16, 256}, {4096, 2048, 32, 128},
      // want clamped from above at 64: 16 tiles give 64, 17 tiles give 60 -> 137 -> 140 rows, 59 chunks
      {8192, 1024, 64, 128}, {8192, 1025, 59, 140},
      // the rows allow fewer chunks than wanted (maxc < want) / more (maxc > want)
      {640, 64, 10, 64}, {960, 64, 15, 64}, {961, 64, 16, 64}, {4096, 64, 64, 64}, {4097, 64, 61, 68},
      // rows per chunk rounded up to 4; after the rounding fewer chunks cover the rows
      {65, 65, 2, 36}, {130, 257, 3, 44},
      // the floor of 4, rows at 0 and 1
      {0, 64, 1, 4}, {1, 1, 1, 4}, {3, 1, 1, 4}, {0, 0, 1, 4},
      // C at 1, 63, 64, 65 and 4096
      {16384, 1, 64, 256}, {64, 63, 1, 64}, {64, 64, 1, 64}, {65, 64, 2, 36}, {128, 65, 2, 64}, {4097, 4096, 16, 260},
      // the benchmark's mel-side rows
      {26912, 512, 64, 424}, {26912, 80, 64, 424},
  };
  for (const Row& r : table) {
    const ChunkPlan p = plan_chunks(r.rows, r.C);
    if (p.nchunks != r.nchunks || p.rows_per_chunk != r.rpc) {
      fprintf(stderr, "plan_chunks(%ld, %d) = (%d, %d), table (%d, %d)\n", r.rows, r.C, p.nchunks, p.rows_per_chunk,
              r.nchunks, r.rpc);
      ++g_failed;
    }
  }
  // what the sizes make of the plan: one pair of doubles per chunk and column; an empty column sum keeps one pair
  CHECK(bn_bytes(5 * 13, 64) == 2 * 64 * 16);
  CHECK(bn_bytes(27 * 161, 64) == 64 * 64 * 16);
  CHECK(colsum_bytes(0, 5) == 5 * 16 && colsum_bytes(5, 0) == 16 && colsum_bytes(0, 0) == 16);
  CHECK(colsum_bytes(4097, 64) == 61 * 64 * 16);
}

static void test_chunk_invariants() {
  const long rows[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 959, 960, 961, 1023, 1024, 1025, 4095,
                       4096, 4097, 4100, 8191, 8192, 26912, 65535, 65536, 1L << 20, (1L << 31) + 7};
  for (long r : rows)
    for (int C = 0; C <= 8200; C += (C < 130 ? 1 : 61)) {
      const ChunkPlan p = plan_chunks(r, C);
      CHECK((long)p.nchunks * p.rows_per_chunk >= r);
      CHECK(p.rows_per_chunk % 4 == 0 && p.rows_per_chunk >= 4);
      CHECK(p.nchunks >= 1 && p.nchunks <= 65535);
      CHECK(p.nchunks <= 64);                                              // the ordered finalize stays short
      CHECK(r == 0 || (long)(p.nchunks - 1) * p.rows_per_chunk < r);         // no empty chunk
    }
}

static void test_colsum_batch() {
  const long rows[] = {1, 37, 64, 65, 961, 4096, 26912};
  const int widths[] = {4, 64, 68, 192, 256, 768, 1024, 1536, 4096, 32768};
  for (long r : rows)
    for (int n = 1; n <= CSB_MAX; ++n) {
      int C[CSB_MAX];
      for (int i = 0; i < n; ++i) C[i] = widths[(i * 7 + n) % 10];
      const ColsumBatchLayout b = colsum_batch(n, C, r);
      CHECK(b.bytes == colsum_batch_bytes(n, C, r));
      CHECK(b.ws_off[0] == 0 && b.tile64[0] == 0 && b.tile32[0] == 0);
      int maxchunks = 1;
      for (int i = 0; i < n; ++i) {
        // every task keeps the plan of its stand-alone sum, and its partials end where the next task's begin
        const ChunkPlan p = plan_chunks(r, C[i]);
        CHECK(b.nchunks[i] == p.nchunks && b.rpc[i] == p.rows_per_chunk);
        const long end = b.ws_off[i] + (long)(colsum_bytes(r, C[i]) / sizeof(double));
        CHECK(colsum_bytes(r, C[i]) == (size_t)p.nchunks * C[i] * 16);
        CHECK(i + 1 < n ? b.ws_off[i + 1] == end : (size_t)end * sizeof(double) == b.bytes);
        CHECK(b.tile64[i + 1] - b.tile64[i] == (C[i] + 63) / 64 && b.tile32[i + 1] - b.tile32[i] == (C[i] + 31) / 32);
        if (p.nchunks > maxchunks) maxchunks = p.nchunks;
      }
      CHECK(b.maxchunks == maxchunks);
    }
}

static void test_conv_sizes() {
  for (int B : {1, 3, 4, 32})
    for (int T : {1, 12, 64, 65, 128, 129, 841, 842})
      for (int C : {1, 16, 64, 65, 68, 128, 256, 258, 512, 640, 768, 2048, 4096}) {
        const size_t s = conv_stats_bytes(B, T, C);
        CHECK(s >= bn_bytes((long)B * T, C));
        CHECK(s >= (size_t)(((long)B * T + 127) / 128) * C * 16);
        for (int k = 1; k <= 17; ++k) {
          for (bool enabled : {false, true}) {
            const ConvFwdStats p = conv_fwd_stats(B, T, C, k, enabled);
            CHECK(p.stats_bytes == s && p.slab_offset >= s && p.slab_offset % 256 == 0 && p.slab_offset < s + 256);
            CHECK((p.tap_split.extra_bytes == 0) == !p.tap_split.on);
            CHECK(p.bytes == p.slab_offset + p.tap_split.extra_bytes);
            CHECK(!p.tap_split.on || (enabled && p.tap_split.extra_bytes == (size_t)k * B * T * C * 4));
          }
          const Extra e = bank_bwd_partials(B, T, C, k);
          CHECK((e.extra_bytes == 0) == !e.on);
          CHECK(!e.on || e.extra_bytes == (size_t)k * B * T * C * 4);
        }
      }
  // both sides of every threshold; 4096 rows = 32 row tiles
  CHECK(conv_tap_split(32, 128, 256, 3, true).on);        // 64 tiles x 3 = 192
  CHECK(!conv_tap_split(32, 128, 256, 2, true).on);       // 64 tiles x 2 = 128 < 192
  CHECK(!conv_tap_split(32, 128, 256, 3, false).on);      // switched off
  CHECK(conv_tap_split(32, 128, 640, 3, true).on);        // 160 tiles < 192
  CHECK(!conv_tap_split(32, 128, 768, 3, true).on);       // 192 tiles: enough on their own
  CHECK(conv_tap_split(32, 128, 68, 6, true).on && !conv_tap_split(32, 128, 64, 6, true).on);      // Cout > 64
  CHECK(!conv_tap_split(32, 128, 258, 3, true).on);       // Cout % 4
  CHECK(conv_tap_split(32, 128, 256, 16, true).on && !conv_tap_split(32, 128, 256, 17, true).on);  // one task per tap
  CHECK(!conv_tap_split(1, 64, 4096, 16, true).on && conv_tap_split(1, 65, 4096, 16, true).on);    // more than 64 rows
  CHECK(conv_tap_split(32, 128, 256, 3, true).extra_bytes == (size_t)3 * 4096 * 256 * 4);
  CHECK(conv_fwd_stats(32, 128, 256, 3, true).bytes == 262144 + 12582912);
  CHECK(conv_fwd_stats(3, 70, 70, 3, true).slab_offset == 4608);       // 4480 bytes of partials, 256-byte aligned
  CHECK(bank_bwd_partials(32, 128, 256, 3).on && !bank_bwd_partials(32, 128, 256, 2).on);
  CHECK(bank_bwd_partials(32, 128, 640, 2).on && !bank_bwd_partials(32, 128, 768, 2).on);
  CHECK(bank_bwd_partials(32, 128, 68, 16).on && !bank_bwd_partials(32, 128, 64, 16).on);
  CHECK(!bank_bwd_partials(1, 64, 4096, 16).on && bank_bwd_partials(1, 65, 4096, 16).on);
  CHECK(!bank_bwd_partials(32, 128, 256, 1).on);
  CHECK(bank_bwd_partials(32, 128, 256, 16).extra_bytes == (size_t)16 * 4096 * 256 * 4);
}

// the composite of an FFTBlock backward.  The weight-gradient workspace must hold the batched column sums too (they run
// there when the caller gives no sums workspace); the sweep reports the smallest shape where they are the larger term.
static void test_fft_block() {
  const gemm_plan::Switches sw(no_env);
  long best = -1;
  int bB = 0, bT = 0, bd = 0, bf = 0;
  auto visit = [&](int B, int T, int d, int f, int k1, int k2) {
    const FftBlockPlan p = fft_block(B, T, d, d / 64, f, k1, k2, sw);
    const int C[8] = {d, d, d, f, d, d, d, 3 * d};
    CHECK(p.sums == colsum_batch_bytes(8, C, (long)B * T));
    CHECK(p.wgrad >= p.sums && p.wgrad >= p.tn_slabs && (p.wgrad == p.sums || p.wgrad == p.tn_slabs));
    CHECK(p.tn_slabs >= (size_t)3 * d * d * 4 && p.tn_slabs >= (size_t)d * f * (k1 > k2 ? k1 : k2) * 4);   // one slab each
    CHECK(p.attn == (size_t)B * (d / 64) * T * 4);
    // the sums one by one (FT_FFT_BATCH_SUMS=0) fit where the batch fits
    CHECK(p.sums >= colsum_bytes((long)B * T, 3 * d) && p.sums >= colsum_bytes((long)B * T, f));
    const long cost = (long)B * T * (f + 9L * d);
    if (p.sums > p.tn_slabs && (best < 0 || cost < best)) {
      best = cost;
      bB = B; bT = T; bd = d; bf = f;
    }
  };
  for (int B : {1, 2, 32})
    for (int T : {1, 37, 64, 65, 128, 129, 500, 841, 960, 961, 1024, 2048})
      for (int d : {64, 128, 256, 384, 512})
        for (int f : {64, 128, 256, 1024, 1536, 4096, 16384, 32704, 32708, 32768, 65536})
          for (int k1 : {1, 3, 9})
            for (int k2 : {1, 3}) visit(B, T, d, f, k1, k2);
  // where the sums can win: one weight-gradient slab (512 or more 64 x 64 tiles: no row split) against 16 chunks
  for (int T = 900; T <= 1030; ++T)
    for (int f = 32000; f <= 32800; f += 4) visit(1, T, 64, f, 1, 1);
  printf("smallest swept FFTBlock whose column sums outgrow its weight-gradient slabs: B=%d T=%d d=%d dfft=%d\n", bB, bT,
         bd, bf);
  CHECK(best > 0);
  CHECK(bB == 1 && bT == 961 && bd == 64 && bf == 32708);       // tests/test_gpu_transformer_routes.py runs this shape
  const FftBlockPlan p = fft_block(1, 961, 64, 1, 32708, 1, 1, sw);
  CHECK(p.sums > p.tn_slabs && p.wgrad == p.sums);
  // 16 chunks x 16 bytes x (9 d + dfft) columns against one slab of 4 d dfft bytes
  CHECK(p.sums == (size_t)16 * 16 * (9 * 64 + 32708) && p.tn_slabs == (size_t)4 * 64 * 32708);
}

int main() {
  test_chunk_table();
  test_chunk_invariants();
  test_colsum_batch();
  test_conv_sizes();
  test_fft_block();
  if (g_failed) {
    fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("reduce_plan: ok\n");
  return 0;
}
