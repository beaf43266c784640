// MelGAN generator for inference on a RAGGED batch of mels (melgan.MelGAN.inference_batch; the definition is DESIGN.md
// section 7, "MelGAN vocoder").  Four kernels: the input convolution, LeakyReLU + transposed convolution in polyphase
// form, the fused residual block, and the output stage.  The panel routine, the arrangements, the staging and the three
// kernels that the HiFi-GAN generator (ft_hifigan.hip) runs too are in ft_voc_tile.h, with the LeakyReLU slope and the
// edge rule as template parameters; the residual block is this file's own.
//
// Common to all of them:
//   * activations are channels-last [row, C] fp32; at the stage whose upsampling so far is `scale`, item b owns rows
//     [b * stride, (b + 1) * stride), stride = (Tmax + tail) * scale, and its own length is L = (len[b] + tail) * scale
//     (tail = the ten appended frames of `inference`, 0 for `forward`).  len[b] is read on the device through
//     ft_item_len (clamped into [1, Tmax]; lens == NULL: every item has Tmax frames);
//   * grid = (tiles of one item, B): every tile starts at an item's row 0, so what a row holds never depends on the
//     batch around it.  A workgroup whose rows all lie at >= L stores nothing and leaves; rows at >= L inside a tile
//     are not stored either, and no kernel ever loads a row at >= L: reflection and the zero rows of the transposed
//     convolution are resolved against L while the input tile is staged, so what lies past an item's length (padding
//     of the mel, NaN, uninitialised memory) never meets arithmetic;
//   * reflection is per item: row -j reads row j, row L - 1 + j reads row L - 1 - j;
//   * every product runs on the exact-fp32 MFMA v_mfma_f32_32x32x2_f32 through ONE routine, mma_panel: D[row][co] +=
//     X[row][k] W[k][co], X a tile in LDS (row stride C + 4 floats: the 16 lanes of a b128 read phase tile the 64
//     banks), W packed [k][CP] in global memory (CP = the output width rounded up to 32, zero columns behind it; the
//     weights of every stage stay L2-resident), activation row on the MFMA's M, output channel on its N: a lane holds one
//     output channel of 16 rows, so each register is stored as 32 consecutive floats.  The k order is a function of
//     the width alone: bit-identical results for an item alone and inside any batch;
//   * a workgroup is 4 or 8 waves, arranged WR (rows) x WC (output-channel tiles); a wave owns RT row tiles of 32 rows, so
//     one weight fragment feeds RT MFMAs.  The plan (plan_rows below) picks the arrangement from the width: narrow
//     stages split the rows between the waves (one 32-channel tile is all there is), wide ones the output channels;
//   * no scratch, no allocation, no synchronisation, no workspace: the activations are the caller's buffers.
#include "ft_voc_tile.h"

namespace {

using namespace ft_voc_tile;

// the input convolution, the transposed convolution and the output stage are the kernels of ft_voc_tile.h at MelGAN's
// slope (0.2), edge rule (reflection) and normalisation; the residual block is this file's own
typedef Lrelu02 Act;

__device__ __forceinline__ float lrelu(float v) { return Act::f(v); }

// ---------------------------------------------------------------------------------------------------
// 3. residual block, ONE launch: out = Ws x + bs + W2 lrelu(W1 * lrelu(reflect_d(x)) + b1) + b2, W1 three taps at
//    dilation d.  LDS: the input tile with d halo rows on either side (LDS row i = input row t0 - d + i, reflected), and
//    the [tile, C] intermediate lrelu(mid), which never reaches memory.  Phase 1 forms mid from the taps at LDS rows r,
//    r + d, r + 2 d; phase 2 sums the 1x1 convolution of mid and the shortcut of the raw x (LDS row r + d) in the same
//    accumulators.  w1: [3][C][CP], w2, ws: [C][CP].
// ---------------------------------------------------------------------------------------------------
constexpr int MAXD = 9;

template <class C>
__global__ __launch_bounds__(C::THREADS) void resblock_kernel(const float* __restrict__ x, const long* __restrict__ lens, int Tmax,
                                                       int tail, int scale, int ch, int CP, int d, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, const float* __restrict__ w2,
                                                       const float* __restrict__ b2, const float* __restrict__ ws,
                                                       const float* __restrict__ bs, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float smem[(2 * C::ROWS + 2 * MAXD) * C::XS];
  const int b = blockIdx.y;
  const long t0 = (long)blockIdx.x * C::ROWS;
  const long L = item_rows(lens, b, Tmax, tail, scale, nullptr);
  if (t0 >= L) return;
  const Wave v = Wave::make<C>();
  const int xrs = ch + 4;
  float* xs = smem;
  float* ms = smem + (C::ROWS + 2 * MAXD) * xrs;
  const long ioff = (long)b * (Tmax + tail) * scale * ch;
  stage_rows<EDGE_REFLECT>(xs, xrs, x + ioff, ch, t0 - d, C::ROWS + 2 * d, L, C::THREADS);
  __syncthreads();
  const int row0 = v.wr * 32 * C::RT;
  for (int ct = v.wc; ct * 32 < ch; ct += C::WC) {
    const int co = 32 * ct + v.l31;
    f32x16 acc[C::RT];
    fill<C::RT>(acc, b1[co]);
    for (int tap = 0; tap < 3; ++tap)
      mma_panel<C::RT, Act>(acc, xs + (row0 + v.l31 + tap * d) * xrs + 4 * v.hf, xrs,
                             w1 + ((long)tap * ch + 4 * v.hf) * CP + co, CP, ch);
    if (co < ch) {
#pragma unroll
      for (int r = 0; r < C::RT; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) ms[(row0 + 32 * r + crow(e, v.hf)) * xrs + co] = lrelu(acc[r][e]);
    }
  }
  __syncthreads();
  float* obase = out + ioff + t0 * ch;
  for (int ct = v.wc; ct * 32 < ch; ct += C::WC) {
    const int co = 32 * ct + v.l31;
    f32x16 acc[C::RT];
    fill<C::RT>(acc, b2[co] + bs[co]);
    mma_panel<C::RT, NoAct>(acc, ms + (row0 + v.l31) * xrs + 4 * v.hf, xrs, w2 + (long)(4 * v.hf) * CP + co, CP, ch);
    mma_panel<C::RT, NoAct>(acc, xs + (row0 + v.l31 + d) * xrs + 4 * v.hf, xrs, ws + (long)(4 * v.hf) * CP + co, CP, ch);
    if (co < ch) {
#pragma unroll
      for (int r = 0; r < C::RT; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = row0 + 32 * r + crow(e, v.hf);
          if (t0 + row < L) obase[(long)row * ch + co] = acc[r][e];
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// the launch plan: the arrangement per staged width (file header).  LDS per workgroup in brackets.
// ---------------------------------------------------------------------------------------------------
// Wide stages have few rows and a long contraction: there the grid is widened (grid.z: channel-tile groups of the input
// convolution, one phase per workgroup of the 8-phase transposed convolutions) and the 256-channel tiles, which fill
// the LDS of a CU alone, get eight waves.  The narrow residual blocks run four workgroups per CU (39 / 40 KB): against
// 128-row tiles at 75 KB (two per CU) that measured -25 % at 32 channels and -21 % at 64 (profiles/melgan.txt).
typedef Cfg<128, 1, 4, 2> In128;       // input convolution: 64 rows, waves over the channel tiles          [37 KB]
typedef Cfg<64, 4, 1, 1> Up64;         // transposed convolution by cin: 128 rows, waves over the rows      [35 KB]
typedef Cfg<128, 2, 2, 2> Up128;       //   128 rows, 2 x 2                                                 [68 KB]
typedef Cfg<256, 1, 4, 2> Up256;       //   64 rows, waves over the channel tiles                           [68 KB]
typedef Cfg<512, 1, 8, 2> Up512;       //   64 rows, eight waves over the channel tiles                     [134 KB]
typedef Cfg<32, 4, 1, 1> Rb32;         // residual block by width: 128 rows, waves over the rows            [39 KB]
typedef Cfg<64, 2, 2, 1> Rb64;         //   64 rows, 2 x 2                                                  [40 KB]
typedef Cfg<128, 1, 4, 2> Rb128;       //   64 rows, waves over the channel tiles                           [77 KB]
typedef Cfg<256, 1, 8, 2> Rb256;       //   64 rows, eight waves over the channel tiles                     [152 KB]

int plan_rows(int kind, int c) {
  if (c < 8 || c % 8) return 0;
  switch (kind) {
    case 0: return c <= 128 ? In128::ROWS : 0;
    case 1: return c <= 64 ? Up64::ROWS : c <= 128 ? Up128::ROWS : c <= 256 ? Up256::ROWS : c <= 512 ? Up512::ROWS : 0;
    case 2: return c <= 32 ? Rb32::ROWS : c <= 64 ? Rb64::ROWS : c <= 128 ? Rb128::ROWS : c <= 256 ? Rb256::ROWS : 0;
    case 3: return c <= OUT_CMAX ? OUT_TILE : 0;
  }
  return 0;
}

}  // namespace

extern "C" {

int ft_melgan_tile_rows(int kind, int c) { return plan_rows(kind, c); }

int ft_melgan_conv_in(const float* mel, const long* lens, int B, int n_mels, int Tmax, int tail, float pad_value,
                      const float* w, const float* bias, int cout, float* out, int* err_flag, void* stream) {
  const int rows = plan_rows(0, n_mels);
  FT_REQUIRE(rows > 0, "melgan_conv_in: n_mels %d must be a multiple of 8 in 8..128", n_mels);
  FT_REQUIRE(B >= 1 && Tmax >= 1 && tail >= 0 && cout >= 1 && B <= 65535, "melgan_conv_in: bad dims");
  FT_REQUIRE(tail == 0 || tail >= 4, "melgan_conv_in: a tail shorter than the reflection is not supported");
  FT_REQUIRE(tail + Tmax >= 4, "melgan_conv_in: fewer than 4 frames cannot be reflected by 3");
  FT_REQUIRE(mel && w && bias && out, "melgan_conv_in: null pointer");
  const int groups = ft_cdiv(ft_cdiv(cout, 32), In128::WC);
  const dim3 grid(ft_cdiv(Tmax + tail, rows), B, groups < 4 ? groups : 4);
  hipLaunchKernelGGL((conv_in_kernel<In128, EDGE_REFLECT, true>), grid, dim3(In128::THREADS), 0, (hipStream_t)stream, mel, lens, Tmax, tail, pad_value, n_mels,
                     w, bias, cout, (cout + 31) / 32 * 32, out, err_flag);
  return ft_check_launch("melgan_conv_in");
}

int ft_melgan_upsample(const float* x, const long* lens, int B, int Tmax, int tail, int scale, int cin, int cout,
                       int stride, const float* w, const float* bias, float* out, void* stream) {
  const int rows = plan_rows(1, cin);
  FT_REQUIRE(rows > 0, "melgan_upsample: cin %d must be a multiple of 8 in 8..512", cin);
  FT_REQUIRE(B >= 1 && Tmax >= 1 && tail >= 0 && scale >= 1 && cout >= 1 && B <= 65535, "melgan_upsample: bad dims");
  FT_REQUIRE(stride >= 2 && stride % 2 == 0 && stride <= 64, "melgan_upsample: stride %d must be even (k = 2 stride, padding = stride / 2)",
             stride);
  FT_REQUIRE(x && w && bias && out && aligned16(x), "melgan_upsample: null or misaligned pointer");
  const dim3 grid(ft_cdiv((long)(Tmax + tail) * scale + 1, rows), B, stride > 2 ? stride : 1);
  const int CP = (cout + 31) / 32 * 32;
  hipStream_t st = (hipStream_t)stream;
#define FT_UP(CFG) \
  hipLaunchKernelGGL((upsample_kernel<CFG, Act>), grid, dim3(CFG::THREADS), 0, st, x, lens, Tmax, tail, scale, cin, cout, CP, stride, w, bias, out)
  if (cin <= 64) FT_UP(Up64);
  else if (cin <= 128) FT_UP(Up128);
  else if (cin <= 256) FT_UP(Up256);
  else FT_UP(Up512);
#undef FT_UP
  return ft_check_launch("melgan_upsample");
}

int ft_melgan_resblock(const float* x, const long* lens, int B, int Tmax, int tail, int scale, int ch, int dilation,
                       const float* w1, const float* b1, const float* w2, const float* b2, const float* ws,
                       const float* bs, float* out, void* stream) {
  const int rows = plan_rows(2, ch);
  FT_REQUIRE(rows > 0, "melgan_resblock: %d channels must be a multiple of 8 in 8..256", ch);
  FT_REQUIRE(B >= 1 && Tmax >= 1 && tail >= 0 && scale >= 1 && B <= 65535, "melgan_resblock: bad dims");
  FT_REQUIRE(dilation >= 1 && dilation <= MAXD, "melgan_resblock: dilation %d (1..%d)", dilation, MAXD);
  FT_REQUIRE((long)((lens ? 1 : Tmax) + tail) * scale > dilation, "melgan_resblock: the shortest item cannot be reflected by %d",
             dilation);
  FT_REQUIRE(x && w1 && b1 && w2 && b2 && ws && bs && out && x != out && aligned16(x), "melgan_resblock: null, aliased or "
             "misaligned pointer");
  const dim3 grid(ft_cdiv((long)(Tmax + tail) * scale, rows), B);
  const int CP = (ch + 31) / 32 * 32;
  hipStream_t st = (hipStream_t)stream;
#define FT_RB(CFG)                                                                                                     \
  hipLaunchKernelGGL(resblock_kernel<CFG>, grid, dim3(CFG::THREADS), 0, st, x, lens, Tmax, tail, scale, ch, CP, dilation, w1, b1, w2, \
                     b2, ws, bs, out)
  if (ch <= 32) FT_RB(Rb32);
  else if (ch <= 64) FT_RB(Rb64);
  else if (ch <= 128) FT_RB(Rb128);
  else FT_RB(Rb256);
#undef FT_RB
  return ft_check_launch("melgan_resblock");
}

int ft_melgan_conv_out(const float* x, const long* lens, int B, int Tmax, int tail, int scale, int ch, const float* w,
                       float bias, float* wav, short* wav_i16, void* stream) {
  FT_REQUIRE(plan_rows(3, ch) > 0, "melgan_conv_out: %d channels must be a multiple of 8 in 8..32", ch);
  FT_REQUIRE(B >= 1 && Tmax >= 1 && tail >= 0 && scale >= 4 && B <= 65535, "melgan_conv_out: bad dims");
  FT_REQUIRE(x && w && wav && wav_i16 && aligned16(x), "melgan_conv_out: null or misaligned pointer");
  const dim3 grid(ft_cdiv((long)Tmax * scale, OUT_TILE), B);
  hipLaunchKernelGGL((conv_out_kernel<Act, EDGE_REFLECT>), grid, dim3(256), 0, (hipStream_t)stream, x, lens, Tmax, tail, scale, ch, w, bias, wav,
                     wav_i16);
  return ft_check_launch("melgan_conv_out");
}

}  // extern "C"
