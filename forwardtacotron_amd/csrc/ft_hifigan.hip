// HiFi-GAN generator for inference on a RAGGED batch of mels (hifigan.HiFiGAN.inference_batch; the definition is
// DESIGN.md section 7, "HiFi-GAN vocoder").  The layout and the rules are those of ft_melgan.hip's header, with tail = 0
// and ZERO edges in place of reflection: channels-last rows, item b at stride Tmax * scale with its own L = len[b] * scale
// read on the device, grid = (tiles of one item, B), workgroups wholly past L leave, rows past L are neither loaded nor
// stored, the zero rows outside [0, L) are resolved while a tile is staged into LDS, every product runs through
// mma_panel in a k order that is a function of the widths and taps alone, no scratch, no workspace, no atomics.
//
// The input convolution, the transposed convolution and the output stage are the kernels of ft_voc_tile.h at HiFi-GAN's
// parameters (no normalisation, slope 0.1 / 0.01, zero edges).  This file's own are the residual convolution and the
// fused pair of ResBlock1.
#include "ft_voc_tile.h"

namespace {

using namespace ft_voc_tile;

typedef Lrelu01 Act;

// how a finished output value reaches memory.  res_mode: 0 nothing is added, 1 the tile's own centre row (raw x, from
// LDS), 2 res[row] from memory.  acc_mode: 0 store, 1 out += value, 2 out = (out + value) / nk -- the average over the nk
// parallel residual blocks of a stage: block 0's last launch stores, the later ones add, the last one divides.  The
// launches of one call are ordered on one stream, so the sum is formed with j ascending, as the definition's is.
__device__ __forceinline__ void emit(float v, float own, const float* __restrict__ res, long at, int res_mode, int acc_mode,
                                     float nk, float* __restrict__ out) {
  if (res_mode == 1) v += own;
  else if (res_mode == 2) v += res[at];
  if (acc_mode >= 1) v = out[at] + v;
  if (acc_mode == 2) v = v / nk;
  out[at] = v;
}

// ---------------------------------------------------------------------------------------------------
// 3. residual convolution: out = res + bias + conv_{k, d}(lrelu(x)), k odd taps at dilation d, zero padding d (k - 1) / 2.
//    LDS row i = input row t0 - halo + i (zeros outside [0, L)); output row r takes the taps at LDS rows r + tap d.
//    w: [k][C][CP].  ResBlock2's convolutions are this kernel with res_mode 1; ResBlock1's are two launches of it where
//    the fused pair below does not fit or loses.
// ---------------------------------------------------------------------------------------------------
constexpr int MAXHALO = 40;             // d (k - 1) / 2 <= 40: (64 + 80) rows of 256 channels are 146 KB of the CU's 160 KB
constexpr int MAXK = 11;

template <class C>
__global__ __launch_bounds__(C::THREADS) void resconv_kernel(const float* __restrict__ x, const long* __restrict__ lens, int Tmax,
                                                      int scale, int ch, int CP, int k, int d, const float* __restrict__ w,
                                                      const float* __restrict__ bias, const float* __restrict__ res,
                                                      int res_mode, int acc_mode, float nk, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xs[(C::ROWS + 2 * MAXHALO) * C::XS];
  const int b = blockIdx.y;
  const long t0 = (long)blockIdx.x * C::ROWS;
  const long L = item_rows(lens, b, Tmax, 0, scale, nullptr);
  if (t0 >= L) return;
  const Wave v = Wave::make<C>();
  const int xrs = ch + 4, halo = d * (k - 1) / 2;
  const long ioff = (long)b * Tmax * scale * ch;
  stage_rows<EDGE_ZERO>(xs, xrs, x + ioff, ch, t0 - halo, C::ROWS + 2 * halo, L, C::THREADS);
  __syncthreads();
  const int row0 = v.wr * 32 * C::RT;
  for (int ct = v.wc; ct * 32 < ch; ct += C::WC) {
    const int co = 32 * ct + v.l31;
    f32x16 acc[C::RT];
    fill<C::RT>(acc, bias[co]);
    for (int tap = 0; tap < k; ++tap)
      mma_panel<C::RT, Act>(acc, xs + (row0 + v.l31 + tap * d) * xrs + 4 * v.hf, xrs, w + ((long)tap * ch + 4 * v.hf) * CP + co,
                            CP, ch);
    if (co < ch) {
#pragma unroll
      for (int r = 0; r < C::RT; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = row0 + 32 * r + crow(e, v.hf);
          if (t0 + row < L)
            emit(acc[r][e], xs[(row + halo) * xrs + co], res, ioff + (t0 + row) * ch + co, res_mode, acc_mode, nk, out);
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// 3b. the fused pair of ResBlock1, ONE launch: out = x + b2 + conv_{k, 1}(lrelu(mid)), mid = b1 + conv_{k, d}(lrelu(x)),
//    with mid ZERO outside [0, L) (the second convolution's padding pads the first one's output).  The MFMA forms C::ROWS
//    rows of mid: item rows t0 - h2 .. t0 - h2 + ROWS - 1, h2 = (k - 1) / 2, which stay in LDS as lrelu(mid); a tile's
//    output is the ROWS - 2 h2 rows whose taps they cover.  LDS row i of x = item row t0 - h2 - h1 + i, h1 = d (k - 1) / 2.
//    The second product runs over all ROWS rows of the MFMA tile; those at >= ROWS - 2 h2 read LDS rows behind mid (inside
//    the allocation, whatever they hold) and are not stored: a row of the product depends on its own row of A alone.
// ---------------------------------------------------------------------------------------------------
constexpr int PAIR_H1 = 25;             // d (k - 1) / 2 of the first convolution: the published (11, 5)

template <class C>
__global__ __launch_bounds__(C::THREADS) void respair_kernel(const float* __restrict__ x, const long* __restrict__ lens, int Tmax,
                                                      int scale, int ch, int CP, int k, int d, const float* __restrict__ w1,
                                                      const float* __restrict__ b1, const float* __restrict__ w2,
                                                      const float* __restrict__ b2, int acc_mode, float nk,
                                                      float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float smem[(2 * C::ROWS + 2 * PAIR_H1 + MAXK - 1) * C::XS];
  const int h2 = (k - 1) / 2, h1 = d * h2, TO = C::ROWS - 2 * h2;
  const int b = blockIdx.y;
  const long t0 = (long)blockIdx.x * TO;
  const long L = item_rows(lens, b, Tmax, 0, scale, nullptr);
  if (t0 >= L) return;
  const Wave v = Wave::make<C>();
  const int xrs = ch + 4;
  float* xs = smem;
  float* ms = smem + (C::ROWS + 2 * PAIR_H1) * xrs;
  const long ioff = (long)b * Tmax * scale * ch;
  stage_rows<EDGE_ZERO>(xs, xrs, x + ioff, ch, t0 - h2 - h1, C::ROWS + 2 * h1, L, C::THREADS);
  __syncthreads();
  const int row0 = v.wr * 32 * C::RT;
  for (int ct = v.wc; ct * 32 < ch; ct += C::WC) {
    const int co = 32 * ct + v.l31;
    f32x16 acc[C::RT];
    fill<C::RT>(acc, b1[co]);
    for (int tap = 0; tap < k; ++tap)
      mma_panel<C::RT, Act>(acc, xs + (row0 + v.l31 + tap * d) * xrs + 4 * v.hf, xrs, w1 + ((long)tap * ch + 4 * v.hf) * CP + co,
                            CP, ch);
    if (co < ch) {
#pragma unroll
      for (int r = 0; r < C::RT; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = row0 + 32 * r + crow(e, v.hf);
          const long t = t0 - h2 + m;
          ms[m * xrs + co] = (t >= 0 && t < L) ? Act::f(acc[r][e]) : 0.f;
        }
    }
  }
  __syncthreads();
  for (int ct = v.wc; ct * 32 < ch; ct += C::WC) {
    const int co = 32 * ct + v.l31;
    f32x16 acc[C::RT];
    fill<C::RT>(acc, b2[co]);
    for (int tap = 0; tap < k; ++tap)
      mma_panel<C::RT, NoAct>(acc, ms + (row0 + v.l31 + tap) * xrs + 4 * v.hf, xrs, w2 + ((long)tap * ch + 4 * v.hf) * CP + co,
                              CP, ch);
    if (co < ch) {
#pragma unroll
      for (int r = 0; r < C::RT; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = row0 + 32 * r + crow(e, v.hf);
          if (row < TO && t0 + row < L)
            emit(acc[r][e], xs[(row + h2 + h1) * xrs + co], nullptr, ioff + (t0 + row) * ch + co, 1, acc_mode, nk, out);
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// the launch plan: the arrangement per staged width.  LDS per workgroup in brackets.
// ---------------------------------------------------------------------------------------------------
typedef Cfg<128, 1, 4, 2> In128;       // input convolution: 64 rows, waves over the channel tiles          [37 KB]
typedef Cfg<64, 4, 1, 1> Up64;         // transposed convolution by cin: 128 rows, waves over the rows      [35 KB]
typedef Cfg<128, 2, 2, 2> Up128;       //   128 rows, 2 x 2                                                 [68 KB]
typedef Cfg<256, 1, 4, 2> Up256;       //   64 rows, waves over the channel tiles                           [68 KB]
typedef Cfg<512, 1, 8, 2> Up512;       //   64 rows, eight waves over the channel tiles                     [134 KB]
typedef Cfg<32, 4, 1, 1> Rc32;         // residual convolution by width: 128 rows, waves over the rows      [30 KB]
typedef Cfg<64, 2, 2, 1> Rc64;         //   64 rows, 2 x 2                                                  [39 KB]
typedef Cfg<128, 1, 4, 2> Rc128;       //   64 rows, waves over the channel tiles                           [76 KB]
typedef Cfg<256, 1, 8, 2> Rc256;       //   64 rows, eight waves over the channel tiles                     [146 KB]
typedef Cfg<32, 4, 1, 1> Rp32;         // fused pair by width: 128 mid rows, waves over the rows            [45 KB]
typedef Cfg<64, 4, 2, 1> Rp64;         //   128 mid rows, eight waves, 4 x 2                                [84 KB]
// (no fused pair above 64 channels: at 128 a 64-row tile is 97 KB and gives 54 rows of 64 at k = 11, at 256 it is over
// the CU's 160 KB)

int plan_rows(int kind, int c) {
  if (c < 8 || c % 8) return 0;
  switch (kind) {
    case 0: return c <= 128 ? In128::ROWS : 0;
    case 1: return c <= 64 ? Up64::ROWS : c <= 128 ? Up128::ROWS : c <= 256 ? Up256::ROWS : c <= 512 ? Up512::ROWS : 0;
    case 2: return c <= 32 ? Rc32::ROWS : c <= 64 ? Rc64::ROWS : c <= 128 ? Rc128::ROWS : c <= 256 ? Rc256::ROWS : 0;
    case 3: return c <= OUT_CMAX ? OUT_TILE : 0;
    case 4: return c <= 32 ? Rp32::ROWS : c <= 64 ? Rp64::ROWS : 0;       // mid rows; a tile's output is ROWS - (k - 1)
  }
  return 0;
}

}  // namespace

extern "C" {

int ft_hifigan_tile_rows(int kind, int c) { return plan_rows(kind, c); }

int ft_hifigan_conv_in(const float* mel, const long* lens, int B, int n_mels, int Tmax, const float* w, const float* bias,
                       int cout, float* out, int* err_flag, void* stream) {
  const int rows = plan_rows(0, n_mels);
  FT_REQUIRE(rows > 0, "hifigan_conv_in: n_mels %d must be a multiple of 8 in 8..128", n_mels);
  FT_REQUIRE(B >= 1 && Tmax >= 1 && cout >= 1 && B <= 65535, "hifigan_conv_in: bad dims");
  FT_REQUIRE(mel && w && bias && out, "hifigan_conv_in: null pointer");
  const int groups = ft_cdiv(ft_cdiv(cout, 32), In128::WC);
  const dim3 grid(ft_cdiv(Tmax, rows), B, groups < 4 ? groups : 4);
  hipLaunchKernelGGL((conv_in_kernel<In128, EDGE_ZERO, false>), grid, dim3(In128::THREADS), 0, (hipStream_t)stream, mel, lens, Tmax, 0,
                     0.f, n_mels, w, bias, cout, (cout + 31) / 32 * 32, out, err_flag);
  return ft_check_launch("hifigan_conv_in");
}

int ft_hifigan_upsample(const float* x, const long* lens, int B, int Tmax, int scale, int cin, int cout, int stride,
                        const float* w, const float* bias, float* out, void* stream) {
  const int rows = plan_rows(1, cin);
  FT_REQUIRE(rows > 0, "hifigan_upsample: cin %d must be a multiple of 8 in 8..512", cin);
  FT_REQUIRE(B >= 1 && Tmax >= 1 && scale >= 1 && cout >= 1 && B <= 65535, "hifigan_upsample: bad dims");
  FT_REQUIRE(stride >= 2 && stride % 2 == 0 && stride <= 64, "hifigan_upsample: stride %d must be even (k = 2 stride, padding = stride / 2)",
             stride);
  FT_REQUIRE(x && w && bias && out && aligned16(x), "hifigan_upsample: null or misaligned pointer");
  const dim3 grid(ft_cdiv((long)Tmax * scale + 1, rows), B, stride > 2 ? stride : 1);
  const int CP = (cout + 31) / 32 * 32;
  hipStream_t st = (hipStream_t)stream;
#define FT_UP(CFG) \
  hipLaunchKernelGGL((upsample_kernel<CFG, Act>), grid, dim3(CFG::THREADS), 0, st, x, lens, Tmax, 0, scale, cin, cout, CP, stride, w, bias, out)
  if (cin <= 64) FT_UP(Up64);
  else if (cin <= 128) FT_UP(Up128);
  else if (cin <= 256) FT_UP(Up256);
  else FT_UP(Up512);
#undef FT_UP
  return ft_check_launch("hifigan_upsample");
}

int ft_hifigan_resconv(const float* x, const long* lens, int B, int Tmax, int scale, int ch, int k, int dilation,
                       const float* w, const float* bias, const float* res, int res_mode, int acc_mode, int nk, float* out,
                       void* stream) {
  const int rows = plan_rows(2, ch);
  FT_REQUIRE(rows > 0, "hifigan_resconv: %d channels must be a multiple of 8 in 8..256", ch);
  FT_REQUIRE(B >= 1 && Tmax >= 1 && scale >= 1 && B <= 65535, "hifigan_resconv: bad dims");
  FT_REQUIRE(k >= 1 && k <= MAXK && k % 2 == 1, "hifigan_resconv: %d taps (odd, 1..%d)", k, MAXK);
  FT_REQUIRE(dilation >= 1 && dilation * (k - 1) / 2 <= MAXHALO, "hifigan_resconv: dilation %d with %d taps needs a halo of %d rows (at most %d)",
             dilation, k, dilation * (k - 1) / 2, MAXHALO);
  FT_REQUIRE(res_mode >= 0 && res_mode <= 2 && (res_mode != 2 || res) && acc_mode >= 0 && acc_mode <= 2 && nk >= 1,
             "hifigan_resconv: bad res_mode / acc_mode / nk");
  FT_REQUIRE(x && w && bias && out && x != out && aligned16(x), "hifigan_resconv: null, aliased or misaligned pointer");
  const dim3 grid(ft_cdiv((long)Tmax * scale, rows), B);
  const int CP = (ch + 31) / 32 * 32;
  hipStream_t st = (hipStream_t)stream;
#define FT_RC(CFG)                                                                                                       \
  hipLaunchKernelGGL(resconv_kernel<CFG>, grid, dim3(CFG::THREADS), 0, st, x, lens, Tmax, scale, ch, CP, k, dilation, w, bias, res, \
                     res_mode, acc_mode, (float)nk, out)
  if (ch <= 32) FT_RC(Rc32);
  else if (ch <= 64) FT_RC(Rc64);
  else if (ch <= 128) FT_RC(Rc128);
  else FT_RC(Rc256);
#undef FT_RC
  return ft_check_launch("hifigan_resconv");
}

int ft_hifigan_respair(const float* x, const long* lens, int B, int Tmax, int scale, int ch, int k, int dilation,
                       const float* w1, const float* b1, const float* w2, const float* b2, int acc_mode, int nk, float* out,
                       void* stream) {
  const int rows = plan_rows(4, ch);
  FT_REQUIRE(rows > 0, "hifigan_respair: %d channels must be a multiple of 8 in 8..64 (wider pairs run as two launches)", ch);
  FT_REQUIRE(B >= 1 && Tmax >= 1 && scale >= 1 && B <= 65535, "hifigan_respair: bad dims");
  FT_REQUIRE(k >= 3 && k <= MAXK && k % 2 == 1, "hifigan_respair: %d taps (odd, 3..%d)", k, MAXK);
  FT_REQUIRE(dilation >= 1 && dilation * (k - 1) / 2 <= PAIR_H1, "hifigan_respair: dilation %d with %d taps needs a halo of %d rows (at most %d)",
             dilation, k, dilation * (k - 1) / 2, PAIR_H1);
  FT_REQUIRE(acc_mode >= 0 && acc_mode <= 2 && nk >= 1, "hifigan_respair: bad acc_mode / nk");
  FT_REQUIRE(x && w1 && b1 && w2 && b2 && out && x != out && aligned16(x), "hifigan_respair: null, aliased or misaligned pointer");
  const dim3 grid(ft_cdiv((long)Tmax * scale, rows - (k - 1)), B);
  const int CP = (ch + 31) / 32 * 32;
  hipStream_t st = (hipStream_t)stream;
#define FT_RP(CFG)                                                                                                          \
  hipLaunchKernelGGL(respair_kernel<CFG>, grid, dim3(CFG::THREADS), 0, st, x, lens, Tmax, scale, ch, CP, k, dilation, w1, b1, w2, b2, \
                     acc_mode, (float)nk, out)
  if (ch <= 32) FT_RP(Rp32);
  else FT_RP(Rp64);
#undef FT_RP
  return ft_check_launch("hifigan_respair");
}

int ft_hifigan_conv_out(const float* x, const long* lens, int B, int Tmax, int scale, int ch, const float* w, float bias,
                        float* wav, short* wav_i16, void* stream) {
  FT_REQUIRE(plan_rows(3, ch) > 0, "hifigan_conv_out: %d channels must be a multiple of 8 in 8..32", ch);
  FT_REQUIRE(B >= 1 && Tmax >= 1 && scale >= 1 && B <= 65535, "hifigan_conv_out: bad dims");
  FT_REQUIRE(x && w && wav && wav_i16 && aligned16(x), "hifigan_conv_out: null or misaligned pointer");
  const dim3 grid(ft_cdiv((long)Tmax * scale, OUT_TILE), B);
  hipLaunchKernelGGL((conv_out_kernel<Lrelu001, EDGE_ZERO>), grid, dim3(256), 0, (hipStream_t)stream, x, lens, Tmax, 0, scale, ch, w,
                     bias, wav, wav_i16);
  return ft_check_launch("hifigan_conv_out");
}

}  // extern "C"
