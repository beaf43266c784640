// What a launch of a GAN vocoder kernel (ft_voc_tile.h, ft_melgan.hip, ft_hifigan.hip) will be, decided on the host in
// plain C++ (no HIP header, no device code, no getenv): the workgroup arrangement per kernel kind and staged width, the
// rows, threads and static LDS bytes that follow from it, the limits on both sides of the C boundary, the fused-or-two-
// launches rule of HiFi-GAN's ResBlock1 pair, and the grid of every kind.  Cfg<...> (ft_voc_tile.h) is instantiated from
// these arrangements and the kernels size their __shared__ arrays with lds_floats below, so the bytes reported here are
// the bytes a kernel allocates.  Every launcher, ft_melgan_tile_rows / ft_hifigan_tile_rows and ft_voc_plan read ONE value
// from here; tests/test_voc_plan_cpu.py and tests/cpp/voc_plan_main.cpp hold it to a hand-written table without a GPU.
#pragma once

namespace voc_plan {

// ------------------------------------------------------------------------------------------------------------------
// kinds.  0..4 are the `kind` of ft_hifigan_tile_rows; ft_melgan_tile_rows has 0..3 with its residual block at 2.
enum Kind { CONV_IN = 0, UPSAMPLE = 1, RESCONV = 2, CONV_OUT = 3, RESPAIR = 4, RESBLOCK = 5, KINDS = 6 };

// ------------------------------------------------------------------------------------------------------------------
// limits
constexpr int LDS_BYTES = 160 * 1024;            // of one CU
constexpr int IN_TAPS = 7;                       // the input and the output convolution
constexpr int REFLECT_MIN = IN_TAPS / 2 + 1;     // rows an item (MelGAN: and its tail) needs for their reflection by 3
constexpr int MAX_TAPS = 11;                     // resconv / respair: k odd, at most this
constexpr int MAX_HALO = 40;                     // resconv: dilation (k - 1) / 2 rows on either side of a tile
constexpr int PAIR_HALO = 25;                    // respair: the same for its first convolution (the published (11, 5))
constexpr int MAX_DILATION = 9;                  // resblock (MelGAN): three taps at dilation 1..9
constexpr int MAX_STRIDE = 64;                   // transposed convolution: even, k = 2 stride, padding = stride / 2
constexpr int MAX_BATCH = 65535;                 // grid.y
constexpr int OUT_ROWS = 256;                    // rows the output stage stages: samples t0 - 3 .. t0 + 252
constexpr int OUT_TILE = OUT_ROWS - (IN_TAPS - 1);      // samples it writes
constexpr int OUT_CMAX = 32;
constexpr int MAX_Z = 4;                         // conv_in: channel-tile groups on grid.z

constexpr bool taps_ok(int k, int kmin) { return k >= kmin && k <= MAX_TAPS && k % 2 == 1; }
constexpr int halo(int k, int d) { return d * (k - 1) / 2; }
constexpr bool stride_ok(int s) { return s >= 2 && s % 2 == 0 && s <= MAX_STRIDE; }

// ------------------------------------------------------------------------------------------------------------------
// arrangements: cmax the widest input a workgroup stages, wr x wc waves (rows x output-channel tiles), rt row tiles of 32
// rows per wave.  Narrow stages split the rows between the waves (one 32-channel tile is all there is), wide ones the
// output channels; the 256- and 512-channel tiles, which fill the LDS of a CU alone, get eight waves.  The narrow residual
// kernels run four workgroups per CU: against 128-row tiles at twice the LDS that measured -25 % at 32 channels and -21 %
// at 64 (profiles/melgan.txt).
struct Arr {
  int cmax, wr, wc, rt;
  constexpr int rows() const { return 32 * rt * wr; }      // output rows (input rows of the transposed convolution) per tile
  constexpr int threads() const { return 64 * wr * wc; }
  constexpr int xs() const { return cmax + 4; }            // LDS row stride in floats at the widest input
};

// per kind, by ascending cmax: width c runs on the first arrangement with c <= cmax
constexpr int MAX_ARRS = 4;
struct Table {
  int n;
  Arr arr[MAX_ARRS];
};
constexpr Table TABLES[KINDS] = {
    /* CONV_IN  */ {1, {{128, 1, 4, 2}}},
    /* UPSAMPLE */ {4, {{64, 4, 1, 1}, {128, 2, 2, 2}, {256, 1, 4, 2}, {512, 1, 8, 2}}},
    /* RESCONV  */ {4, {{32, 4, 1, 1}, {64, 2, 2, 1}, {128, 1, 4, 2}, {256, 1, 8, 2}}},
    /* CONV_OUT */ {1, {{OUT_CMAX, 4, 1, 2}}},
    // no fused pair above 64 channels: at 128 a 64-row tile is 97 KB and gives 54 rows of 64 at k = 11, at 256 it is over
    // the CU's LDS
    /* RESPAIR  */ {2, {{32, 4, 1, 1}, {64, 4, 2, 1}}},
    /* RESBLOCK */ {4, {{32, 4, 1, 1}, {64, 2, 2, 1}, {128, 1, 4, 2}, {256, 1, 8, 2}}},
};
constexpr int count(int kind) { return kind >= 0 && kind < KINDS ? TABLES[kind].n : 0; }
constexpr Arr arr(int kind, int i) { return TABLES[kind].arr[i]; }
constexpr int max_width(int kind) { return count(kind) ? arr(kind, count(kind) - 1).cmax : 0; }

// the arrangement of width c: its index in the kind's table, -1 where the width is not supported (widths are multiples
// of 8, at least 8)
constexpr int pick(int kind, int c) {
  if (c < 8 || c % 8) return -1;
  for (int i = 0; i < count(kind); ++i)
    if (c <= arr(kind, i).cmax) return i;
  return -1;
}

// ------------------------------------------------------------------------------------------------------------------
// static LDS of a kernel in floats: `tiles` blocks of rows() rows plus the kind's extra rows, at the widest row stride;
// the output stage adds its [OUT_ROWS][8] tap products
constexpr int lds_tiles(int kind) { return kind == RESBLOCK || kind == RESPAIR ? 2 : 1; }      // input + intermediate
constexpr int lds_extra_rows(int kind) {
  return kind == CONV_IN    ? IN_TAPS - 1                      // 3 rows on either side
         : kind == UPSAMPLE ? 1                                // input row q0 - 1
         : kind == RESCONV  ? 2 * MAX_HALO
         : kind == RESPAIR  ? 2 * PAIR_HALO + MAX_TAPS - 1     // the first convolution's halo; the rows read behind mid
         : kind == RESBLOCK ? 2 * MAX_DILATION
                            : 0;
}
constexpr int lds_floats(int kind, Arr a) {
  return (lds_tiles(kind) * a.rows() + lds_extra_rows(kind)) * a.xs() + (kind == CONV_OUT ? OUT_ROWS * 8 : 0);
}
constexpr int lds_bytes(int kind, Arr a) { return lds_floats(kind, a) * (int)sizeof(float); }

constexpr bool all_fit() {
  for (int kind = 0; kind < KINDS; ++kind)
    for (int i = 0; i < count(kind); ++i) {
      const Arr a = arr(kind, i);
      if (lds_bytes(kind, a) > LDS_BYTES || (a.wr * a.wc != 4 && a.wr * a.wc != 8)) return false;
      if (i > 0 && a.cmax <= arr(kind, i - 1).cmax) return false;
    }
  return true;
}
static_assert(all_fit(), "every arrangement is four or eight waves and fits the 160 KB of a CU; tables ascend");
static_assert(arr(CONV_OUT, 0).rows() == OUT_ROWS, "the output stage's MFMA tile is its staged rows");

// ------------------------------------------------------------------------------------------------------------------
// what the *_tile_rows queries answer: rows per workgroup tile for width c, 0 where the width is not supported.  conv_out
// counts samples; respair counts rows of the intermediate: a tile's output is that minus k - 1.
constexpr int tile_rows(int kind, int c) {
  const int i = pick(kind, c);
  return i < 0 ? 0 : kind == CONV_OUT ? OUT_TILE : arr(kind, i).rows();
}
constexpr int threads(int kind, int c) {
  const int i = pick(kind, c);
  return i < 0 ? 0 : arr(kind, i).threads();
}

// ------------------------------------------------------------------------------------------------------------------
// ResBlock1's (convs1[m], convs2[m]): one launch with the intermediate in LDS, or two launches of the residual
// convolution.  Per width and (k, d) the winner of the same-process A/B of profiles/hifigan.txt section 2: fused won
// every (k, d) at 32 channels (0.68-0.92 of the two launches' time) and k = 3 at 64 (0.93), and lost k = 7 and 11 at 64
// (1.05, 1.12), where a tile gives 122 / 118 rows of the 128 it computes; d made no difference.  Above 64 channels there
// is no fused kernel (TABLES).
constexpr bool pair_is_fused(int width, int k, int d) {
  if (k < 3 || halo(k, d) > PAIR_HALO) return false;
  return width <= 32 || (width <= max_width(RESPAIR) && k == 3);
}

// ------------------------------------------------------------------------------------------------------------------
// launch geometry.  grid = (tiles of one item, B, z): every tile starts at an item's row 0.  cp: the output width rounded
// up to 32, the row stride of the packed weights.
struct Launch {
  unsigned x, y, z;
  int threads, cp;
};
constexpr long cdiv(long a, long b) { return (a + b - 1) / b; }
constexpr int padded(int cout) { return (cout + 31) / 32 * 32; }

// rows: what one item holds at most; out_rows: rows a tile writes.  -> x tiles
constexpr Launch launch(int kind, int c, long rows, long out_rows, int B, int z, int cout) {
  return Launch{(unsigned)cdiv(rows, out_rows), (unsigned)B, (unsigned)z, threads(kind, c), padded(cout)};
}
// z: groups of wc channel tiles, at most MAX_Z (wide stages have few rows and a long contraction: the grid is widened)
constexpr Launch conv_in(int B, int Tmax, int tail, int n_mels, int cout) {
  const long groups = cdiv(cdiv(cout, 32), arr(CONV_IN, 0).wc);
  return launch(CONV_IN, n_mels, (long)Tmax + tail, tile_rows(CONV_IN, n_mels), B, groups < MAX_Z ? (int)groups : MAX_Z, cout);
}
// a tile is rows() values of q = 0 .. Lin INCLUSIVE (q = Lin still feeds the phases p < stride / 2): one more row.  z: one
// phase per workgroup above stride 2
constexpr Launch upsample(int B, int Tmax, int tail, int scale, int cin, int cout, int stride) {
  return launch(UPSAMPLE, cin, ((long)Tmax + tail) * scale + 1, tile_rows(UPSAMPLE, cin), B, stride > 2 ? stride : 1, cout);
}
// kind: RESBLOCK or RESCONV
constexpr Launch residual(int kind, int B, int Tmax, int tail, int scale, int ch) {
  return launch(kind, ch, ((long)Tmax + tail) * scale, tile_rows(kind, ch), B, 1, ch);
}
constexpr Launch respair(int B, int Tmax, int scale, int ch, int k) {
  return launch(RESPAIR, ch, (long)Tmax * scale, tile_rows(RESPAIR, ch) - (k - 1), B, 1, ch);
}
// (the tail's samples are never formed)
constexpr Launch conv_out(int B, int Tmax, int scale, int ch) {
  return launch(CONV_OUT, ch, (long)Tmax * scale, OUT_TILE, B, 1, 1);
}

// ------------------------------------------------------------------------------------------------------------------
// ft_voc_plan(field, a, b, c): the one value-returning query through which Python reads what it needs of the above
enum Field { F_MAX_TAPS = 0, F_MAX_HALO = 1, F_PAIR_HALO = 2, F_PAIR_IS_FUSED = 3 /* a = width, b = k, c = dilation */ };
constexpr int query(int field, int a, int b, int c) {
  return field == F_MAX_TAPS        ? MAX_TAPS
         : field == F_MAX_HALO      ? MAX_HALO
         : field == F_PAIR_HALO     ? PAIR_HALO
         : field == F_PAIR_IS_FUSED ? (pair_is_fused(a, b, c) ? 1 : 0)
                                    : -1;
}

}  // namespace voc_plan
