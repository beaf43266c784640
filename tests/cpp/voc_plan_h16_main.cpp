// Stand-alone host test of csrc/ft_voc_plan_h16.h (tests/test_hifigan_fp16_cpu.py builds it with the sanitizers and runs
// it): the launch plan of HiFi-GAN's fp16-operand residual convolution against a hand-written table.
//
// Where the table comes from (never from the header under test): the waves and rows are those of the fp32 residual
// convolution; the bytes are (rows + 2 x 40 halo rows) x (staged width + 8) halves x 2, worked out by hand:
// 208 x 40 x 2 = 16,640; 144 x 72 x 2 = 20,736; 144 x 136 x 2 = 39,168; 144 x 264 x 2 = 76,032.
#include <stdio.h>

#include "ft_voc_plan_h16.h"

namespace P = voc_plan_h16;

static int g_failed = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                               \
    }                                                           \
  } while (0)

struct Row {
  int upto, rows, threads, bytes;      // widths up to `upto` (above the row before)
};
static const Row TABLE[] = {{32, 128, 256, 16640}, {64, 64, 256, 20736}, {128, 64, 256, 39168}, {256, 64, 512, 76032}};

static const Row* row_of(int c) {
  if (c < 8 || c % 8) return nullptr;
  for (const Row& r : TABLE)
    if (c <= r.upto) return &r;
  return nullptr;
}

static void test_every_width() {
  for (int c = -8; c <= 300; ++c) {
    const Row* r = row_of(c);
    const int cpad = (c + 15) / 16 * 16;
    const int want[5] = {r ? r->rows : 0, r ? r->bytes : 0, r ? r->threads : 0, r ? r->upto : 0, r ? cpad : 0};
    for (int f = 0; f < 5; ++f)
      if (P::query(f, c) != want[f]) {
        fprintf(stderr, "query(%d, %d) = %d, table %d\n", f, c, P::query(f, c), want[f]);
        ++g_failed;
      }
    CHECK(P::tile_rows(c) == want[0] && P::threads(c) == want[2]);
    CHECK(P::query(-1, c) == -1 && P::query(5, c) == -1);
  }
}

static void test_arrangements() {
  CHECK(P::COUNT == 4 && P::MAX_WIDTH == 256 && P::KSTEP == 16);
  for (int i = 0; i < P::COUNT; ++i) {
    const voc_plan::Arr a = P::ARRS[i];
    CHECK(a.cmax == TABLE[i].upto && a.rows() == TABLE[i].rows && a.threads() == TABLE[i].threads);
    CHECK(P::lds_bytes(a) == TABLE[i].bytes);
    CHECK(TABLE[i].bytes <= 160 * 1024);
    // the fp16 tile is about half the fp32 tile of the same rows: (cmax + 8) halves against (cmax + 4) floats
    CHECK(2 * P::lds_bytes(a) > voc_plan::lds_bytes(voc_plan::RESCONV, voc_plan::arr(voc_plan::RESCONV, i)));
    CHECK(P::lds_bytes(a) < voc_plan::lds_bytes(voc_plan::RESCONV, voc_plan::arr(voc_plan::RESCONV, i)) * 3 / 5);
    // the row stride in dwords is 4 x odd: 16 rows distinct modulo 16 fall on 16 different 16-byte slots of the 64 banks
    CHECK(P::row_halves(a.cmax) % 8 == 0 && (P::row_halves(a.cmax) / 8) % 2 == 1);
  }
  CHECK(2 * TABLE[3].bytes <= 160 * 1024);       // the point of the fp16 tile: two 256-channel workgroups on a CU
  CHECK(P::cpad(8) == 16 && P::cpad(16) == 16 && P::cpad(24) == 32 && P::cpad(40) == 48 && P::cpad(256) == 256);
  for (int c = 8; c <= 256; c += 8) CHECK(P::cpad(c) <= P::ARRS[P::pick(c)].cmax && P::cpad(c) % 16 == 0 && P::cpad(c) - c < 16);
}

static bool same(const voc_plan::Launch& g, unsigned x, unsigned y, int threads, int cp) {
  const bool ok = g.x == x && g.y == y && g.z == 1 && g.threads == threads && g.cp == cp;
  if (!ok) fprintf(stderr, "  launch (%u, %u, %u) x %d, cp %d; table (%u, %u, 1) x %d, cp %d\n", g.x, g.y, g.z, g.threads, g.cp, x, y, threads, cp);
  return ok;
}

static void test_grids() {
  CHECK(same(P::launch(5, 16, 8, 32), 1, 5, 256, 32));        // 128 rows, 128-row tile
  CHECK(same(P::launch(5, 129, 1, 8), 2, 5, 256, 32));
  CHECK(same(P::launch(5, 16, 8, 40), 2, 5, 256, 64));        // 64-row tiles from 40 channels up
  CHECK(same(P::launch(1, 43, 3, 256), 3, 1, 512, 256));      // 129 rows; eight waves
  CHECK(same(P::launch(1, 1 << 20, 256, 8), 1u << 21, 1, 256, 32));
}

int main() {
  test_every_width();
  test_arrangements();
  test_grids();
  if (g_failed) {
    fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("voc_plan_h16: ok\n");
  return 0;
}
