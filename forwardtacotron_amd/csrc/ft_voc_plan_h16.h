// What a launch of HiFi-GAN's fp16-operand residual convolution (ft_hifigan_h16.hip, ft_hifigan_resconv_h16) will be,
// decided on the host in plain C++ like ft_voc_plan.h, whose limits (taps, halo, batch) and grid arithmetic it reuses and
// whose tables it leaves alone: this is a separate table with its own query.  The LDS tile holds fp16 values of
// lrelu(x), so a row is cpad + 8 halves: cpad the width rounded up to the 16 the MFMA contracts at a time (zeros behind
// the width), 8 halves of padding -- the fp32 tile's stride in dwords, (cpad + 8) / 2 = 4 * odd, so the 16 rows of a
// ds_read_b128 lane group (rows distinct modulo 16, 16 bytes each) fall on 16 different 4-bank slots.
// tests/cpp/voc_plan_h16_main.cpp holds this header to a hand-written table without a GPU.
#pragma once

#include "ft_voc_plan.h"

namespace voc_plan_h16 {

using voc_plan::Arr;

constexpr int KSTEP = 16;                        // k of v_mfma_f32_32x32x16_f16
constexpr int ROW_PAD = 8;                       // halves behind the staged width of an LDS row

// by ascending cmax (the staged width, a multiple of KSTEP): the waves and row tiles of ft_voc_plan.h's RESCONV, at half
// the bytes per row.  The 256-channel tile with its 40-row halo is 76,032 bytes: two workgroups fit on a CU.
constexpr int COUNT = 4;
constexpr Arr ARRS[COUNT] = {{32, 4, 1, 1}, {64, 2, 2, 1}, {128, 1, 4, 2}, {256, 1, 8, 2}};
constexpr int MAX_WIDTH = ARRS[COUNT - 1].cmax;

// the contraction of width c: c rounded up to KSTEP
constexpr int cpad(int c) { return (c + KSTEP - 1) / KSTEP * KSTEP; }

// the arrangement of width c: its index, -1 where the width is not supported (multiples of 8 from 8)
constexpr int pick(int c) {
  if (c < 8 || c % 8) return -1;
  for (int i = 0; i < COUNT; ++i)
    if (cpad(c) <= ARRS[i].cmax) return i;
  return -1;
}

// static LDS of the kernel in halves: the tile's rows and the widest halo on either side, at the widest row stride
constexpr int row_halves(int staged) { return staged + ROW_PAD; }
constexpr int lds_halves(Arr a) { return (a.rows() + 2 * voc_plan::MAX_HALO) * row_halves(a.cmax); }
constexpr int lds_bytes(Arr a) { return lds_halves(a) * 2; }

constexpr bool all_fit() {
  for (int i = 0; i < COUNT; ++i) {
    const Arr a = ARRS[i];
    if (lds_bytes(a) > voc_plan::LDS_BYTES || (a.wr * a.wc != 4 && a.wr * a.wc != 8) || a.cmax % KSTEP) return false;
    if (i > 0 && a.cmax <= ARRS[i - 1].cmax) return false;
  }
  return true;
}
static_assert(all_fit(), "every arrangement is four or eight waves, stages a multiple of 16 and fits a CU; the table ascends");
static_assert(2 * lds_bytes(ARRS[COUNT - 1]) <= voc_plan::LDS_BYTES, "two of the widest tiles fit on one CU");

constexpr int tile_rows(int c) { return pick(c) < 0 ? 0 : ARRS[pick(c)].rows(); }
constexpr int threads(int c) { return pick(c) < 0 ? 0 : ARRS[pick(c)].threads(); }

// grid = (tiles of one item, B); cp: the output width rounded up to 32, the column count of the packed weights
constexpr voc_plan::Launch launch(int B, int Tmax, int scale, int ch) {
  return voc_plan::Launch{(unsigned)voc_plan::cdiv((long)Tmax * scale, tile_rows(ch)), (unsigned)B, 1u, threads(ch),
                          voc_plan::padded(ch)};
}

// ft_hifigan_h16_plan(field, c): what Python and the tests read of the above for width c.  An unsupported width answers
// 0, an unknown field -1.
enum Field { F_TILE_ROWS = 0, F_LDS_BYTES = 1, F_THREADS = 2, F_STAGED = 3 /* cmax */, F_CPAD = 4 };
constexpr int query(int field, int c) {
  if (field < F_TILE_ROWS || field > F_CPAD) return -1;
  const int i = pick(c);
  if (i < 0) return 0;
  return field == F_TILE_ROWS   ? ARRS[i].rows()
         : field == F_LDS_BYTES ? lds_bytes(ARRS[i])
         : field == F_THREADS   ? ARRS[i].threads()
         : field == F_STAGED    ? ARRS[i].cmax
                                : cpad(c);
}

}  // namespace voc_plan_h16
