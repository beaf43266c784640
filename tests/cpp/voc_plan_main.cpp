// Stand-alone host test of csrc/ft_voc_plan.h (tests/test_voc_plan_cpu.py builds it with the sanitizers and runs it): the
// GAN vocoders' launch plan -- tile rows, threads and static LDS bytes per arrangement, the limits, the fused-pair rule
// and the grid of every kind -- against a hand-written table.
//
// Where the table comes from (never from the header under test): the rows are what the two plan_rows switches of
// ft_melgan.hip / ft_hifigan.hip answered before the plan moved into the header; the LDS bytes are the __shared__
// expressions of those files worked out by hand ((64 + 6) rows x 132 floats x 4 = 36,960 for the input convolution, ...)
// and equal what the compiler's resource report gives for every kernel (profiles/voc_plan_ab.txt); the pair rule is the
// body hifigan.pair_is_fused had; the grids are the launchers' inline arithmetic on shapes worked out by hand.
#include <stdio.h>

#include <initializer_list>

#include "ft_voc_plan.h"

using namespace voc_plan;

static int g_failed = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                               \
    }                                                           \
  } while (0)

// rows per tile for every width 0..520: multiples of 8 from 8 up to each kind's widest, 0 everywhere else
static int table_rows(int kind, int c) {
  if (c < 8 || c % 8) return 0;
  switch (kind) {
    case CONV_IN: return c <= 128 ? 64 : 0;
    case UPSAMPLE: return c <= 128 ? 128 : c <= 512 ? 64 : 0;
    case RESCONV:
    case RESBLOCK: return c <= 32 ? 128 : c <= 256 ? 64 : 0;
    case CONV_OUT: return c <= 32 ? 250 : 0;
    case RESPAIR: return c <= 64 ? 128 : 0;
  }
  return 0;
}

static void test_tile_rows() {
  for (int kind = 0; kind < KINDS; ++kind)
    for (int c = 0; c <= 520; ++c)
      if (tile_rows(kind, c) != table_rows(kind, c)) {
        fprintf(stderr, "tile_rows(%d, %d) = %d, table %d\n", kind, c, tile_rows(kind, c), table_rows(kind, c));
        ++g_failed;
      }
  // kinds that do not exist, widths below zero
  CHECK(tile_rows(-1, 64) == 0 && tile_rows(KINDS, 64) == 0 && tile_rows(UPSAMPLE, -8) == 0);
}

static void test_arrangements() {
  struct Row {
    const char* name;
    int kind, width;          // the widest width the arrangement serves; width - 8 is served by it too (or by none)
    int bytes, threads;
  };
  const Row table[] = {
      {"In128", CONV_IN, 128, 36960, 256},    {"Up64", UPSAMPLE, 64, 35088, 256},    {"Up128", UPSAMPLE, 128, 68112, 256},
      {"Up256", UPSAMPLE, 256, 67600, 256},   {"Up512", UPSAMPLE, 512, 134160, 512}, {"Rb32", RESBLOCK, 32, 39456, 256},
      {"Rb64", RESBLOCK, 64, 39712, 256},     {"Rb128", RESBLOCK, 128, 77088, 256},  {"Rb256", RESBLOCK, 256, 151840, 512},
      {"Rc32", RESCONV, 32, 29952, 256},      {"Rc64", RESCONV, 64, 39168, 256},     {"Rc128", RESCONV, 128, 76032, 256},
      {"Rc256", RESCONV, 256, 149760, 512},   {"Rp32", RESPAIR, 32, 45504, 256},     {"Rp64", RESPAIR, 64, 85952, 512},
      {"conv_out", CONV_OUT, 32, 45056, 256},
  };
  int seen = 0;
  for (const Row& r : table) {
    const int i = pick(r.kind, r.width);
    CHECK(i >= 0);
    if (i < 0) continue;
    const Arr a = arr(r.kind, i);
    if (lds_bytes(r.kind, a) != r.bytes || a.threads() != r.threads || a.cmax != r.width) {
      fprintf(stderr, "%s: %d bytes, %d threads, cmax %d; table %d, %d, %d\n", r.name, lds_bytes(r.kind, a), a.threads(),
              a.cmax, r.bytes, r.threads, r.width);
      ++g_failed;
    }
    CHECK(r.bytes <= 163840);
    CHECK(threads(r.kind, r.width) == r.threads);
    // one width up is another arrangement or none; the narrowest width of this one is the one below's widest + 8
    CHECK(pick(r.kind, r.width + 8) != i);
    CHECK(i == 0 ? pick(r.kind, 8) == 0 : pick(r.kind, arr(r.kind, i - 1).cmax + 8) == i);
    ++seen;
  }
  int total = 0;
  for (int kind = 0; kind < KINDS; ++kind) total += count(kind);
  CHECK(seen == 16 && total == 16);       // the table names every arrangement there is
  CHECK(threads(RESCONV, 264) == 0 && threads(CONV_IN, 4) == 0);
}

static void test_limits() {
  CHECK(MAX_TAPS == 11 && MAX_HALO == 40 && PAIR_HALO == 25 && MAX_DILATION == 9 && MAX_STRIDE == 64 && MAX_BATCH == 65535);
  CHECK(OUT_ROWS == 256 && OUT_TILE == 250 && OUT_CMAX == 32 && LDS_BYTES == 163840 && IN_TAPS == 7 && REFLECT_MIN == 4);
  CHECK(query(F_MAX_TAPS, 0, 0, 0) == 11 && query(F_MAX_HALO, 0, 0, 0) == 40 && query(F_PAIR_HALO, 0, 0, 0) == 25);
  CHECK(query(4, 0, 0, 0) == -1 && query(-1, 0, 0, 0) == -1);
  const int widest[KINDS] = {128, 512, 256, 32, 64, 256};
  for (int kind = 0; kind < KINDS; ++kind) CHECK(max_width(kind) == widest[kind]);
  CHECK(max_width(-1) == 0 && max_width(KINDS) == 0);
  // taps: odd, from the kind's least to 11
  for (int k = -1; k <= 14; ++k) {
    CHECK(taps_ok(k, 1) == (k >= 1 && k <= 11 && k % 2 == 1));
    CHECK(taps_ok(k, 3) == (k >= 3 && k <= 11 && k % 2 == 1));
  }
  // strides: even, 2..64
  for (int s = -2; s <= 70; ++s) CHECK(stride_ok(s) == (s >= 2 && s <= 64 && s % 2 == 0));
  // halos: the published (k, d) and both sides of the two limits
  CHECK(halo(11, 5) == 25 && halo(7, 12) == 36 && halo(9, 10) == 40 && halo(9, 11) == 44 && halo(11, 8) == 40 && halo(1, 50) == 0);
  CHECK(halo(3, 25) == 25 && halo(3, 26) == 26);
}

static void test_pair_rule() {
  for (int width : {8, 32, 40, 64, 72, 128})
    for (int k : {1, 3, 7, 11})
      for (int d : {1, 3, 5, 12, 13}) {
        bool want;       // hifigan.pair_is_fused as it was
        if (k < 3 || d * (k - 1) / 2 > 25) want = false;
        else want = width <= 32 || (width <= 64 && k == 3);
        if (pair_is_fused(width, k, d) != want || query(F_PAIR_IS_FUSED, width, k, d) != (want ? 1 : 0)) {
          fprintf(stderr, "pair_is_fused(%d, %d, %d) = %d, table %d\n", width, k, d, (int)pair_is_fused(width, k, d), (int)want);
          ++g_failed;
        }
      }
  // spelled out: the halo limit at k = 3 (d = 25 | 26), at k = 11 (d = 5 | 6), the width steps at k = 3 and k = 7
  CHECK(pair_is_fused(32, 3, 25) && !pair_is_fused(32, 3, 26) && pair_is_fused(32, 11, 5) && !pair_is_fused(32, 11, 6));
  CHECK(pair_is_fused(64, 3, 1) && !pair_is_fused(72, 3, 1) && pair_is_fused(32, 7, 3) && !pair_is_fused(40, 7, 3));
  // what is fused has a kernel (taps as the constructor admits them)
  for (int width = 0; width <= 520; ++width)
    for (int k = 1; k <= MAX_TAPS; k += 2)
      for (int d = 1; d <= 13; ++d)
        if (pair_is_fused(width, k, d) && width >= 8 && width % 8 == 0)
          CHECK(tile_rows(RESPAIR, width) > k - 1 && taps_ok(k, 3) && halo(k, d) <= PAIR_HALO);
}

static bool same(const Launch& g, unsigned x, unsigned y, unsigned z, int threads, int cp) {
  const bool ok = g.x == x && g.y == y && g.z == z && g.threads == threads && g.cp == cp;
  if (!ok) fprintf(stderr, "  launch (%u, %u, %u) x %d, cp %d; table (%u, %u, %u) x %d, cp %d\n", g.x, g.y, g.z, g.threads, g.cp, x, y, z, threads, cp);
  return ok;
}

static void test_grids() {
  // input convolution: 64-row tiles over Tmax + tail frames; z = groups of 4 channel tiles, at most 4
  CHECK(same(conv_in(3, 54, 10, 80, 32), 1, 3, 1, 256, 32));           // 64 frames: one tile; 1 channel tile -> 1 group
  CHECK(same(conv_in(3, 55, 10, 80, 128), 2, 3, 1, 256, 128));         // 65 frames: one more; 4 channel tiles -> 1 group
  CHECK(same(conv_in(1, 64, 0, 80, 256), 1, 1, 2, 256, 256));          // 8 channel tiles -> 2 groups
  CHECK(same(conv_in(1, 128, 0, 8, 512), 2, 1, 4, 256, 512));          // 16 channel tiles -> 4 groups
  CHECK(same(conv_in(1, 129, 0, 128, 160), 3, 1, 2, 256, 160));        // 5 channel tiles -> 2 groups
  CHECK(same(conv_in(65535, 1, 0, 80, 1024), 1, 65535, 4, 256, 1024)); // 32 channel tiles: 8 groups, capped at 4
  CHECK(same(conv_in(1, 1, 0, 80, 520), 1, 1, 4, 256, 544));           // 17 channel tiles -> 5 groups, capped; cp rounds up
  // transposed convolution: tiles over q = 0 .. Lin inclusive; z = the phases above stride 2
  CHECK(same(upsample(2, 127, 0, 1, 64, 32, 2), 1, 2, 1, 256, 32));    // Lin + 1 = 128 rows: one 128-row tile
  CHECK(same(upsample(2, 128, 0, 1, 64, 32, 2), 2, 2, 1, 256, 32));    // Lin = 128: q = Lin opens a second tile
  CHECK(same(upsample(2, 22, 10, 4, 128, 64, 4), 2, 2, 4, 256, 64));   // (22 + 10) * 4 = 128 rows + 1; stride 4 -> z = 4
  CHECK(same(upsample(4, 33, 0, 1, 512, 256, 8), 1, 4, 8, 512, 256));  // 64-row tiles, 34 rows; eight waves; z = 8
  CHECK(same(upsample(4, 64, 0, 1, 512, 250, 8), 2, 4, 8, 512, 256));  // 65 rows
  CHECK(same(upsample(1, 63, 0, 1, 256, 128, 64), 1, 1, 64, 256, 128));
  // residual kernels: Tmax * scale a whole number of tiles, and one more row
  for (int kind : {RESCONV, RESBLOCK}) {
    CHECK(same(residual(kind, 5, 16, 0, 8, 32), 1, 5, 1, 256, 32));    // 128 rows, 128-row tile
    CHECK(same(residual(kind, 5, 6, 10, 8, 32), 1, 5, 1, 256, 32));    // the tail counts
    CHECK(same(residual(kind, 5, 129, 0, 1, 32), 2, 5, 1, 256, 32));
    CHECK(same(residual(kind, 5, 16, 0, 8, 64), 2, 5, 1, 256, 64));    // 64-row tiles from 40 channels up
    CHECK(same(residual(kind, 5, 16, 0, 8, 40), 2, 5, 1, 256, 64));
    CHECK(same(residual(kind, 1, 43, 0, 3, 256), 3, 1, 1, 512, 256));  // 129 rows; eight waves
    CHECK(same(residual(kind, 1, 1 << 20, 0, 256, 8), 1u << 21, 1, 1, 256, 32));       // 2^28 rows of an item
  }
  // fused pair: a tile writes 128 - (k - 1) rows
  CHECK(same(respair(2, 126, 1, 32, 3), 1, 2, 1, 256, 32));
  CHECK(same(respair(2, 127, 1, 32, 3), 2, 2, 1, 256, 32));
  CHECK(same(respair(2, 118, 1, 64, 11), 1, 2, 1, 512, 64));
  CHECK(same(respair(2, 119, 1, 64, 11), 2, 2, 1, 512, 64));
  CHECK(same(respair(2, 59, 4, 48, 7), 2, 2, 1, 512, 64));             // 236 rows in tiles of 122
  // output stage: 250 samples per tile over Tmax * scale (no tail)
  CHECK(same(conv_out(7, 125, 2, 32), 1, 7, 1, 256, 32));
  CHECK(same(conv_out(7, 251, 1, 8), 2, 7, 1, 256, 32));
  CHECK(same(conv_out(1, 23, 256, 32), 24, 1, 1, 256, 32));            // 5888 samples = 23.6 tiles
}

int main() {
  test_tile_rows();
  test_arrangements();
  test_limits();
  test_pair_rule();
  test_grids();
  if (g_failed) {
    fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("voc_plan: ok\n");
  return 0;
}
