// MelGAN generator for inference on a RAGGED batch of mels (melgan.MelGAN.inference_batch; the definition is DESIGN.md
// section 7, "MelGAN vocoder").  Four kernels: the input convolution, LeakyReLU + transposed convolution in polyphase
// form, the fused residual block, and the output stage.  The panel routine, the staging and the three kernels that the
// HiFi-GAN generator (ft_hifigan.hip) runs too are in ft_voc_tile.h, with the LeakyReLU slope and the edge rule as
// template parameters, and their launchers in ft_voc_launch.h; the residual block is this file's own.
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
//     one weight fragment feeds RT MFMAs.  The plan (ft_voc_plan.h, host-only: the arrangements, their LDS bytes, every
//     limit and every grid) picks the arrangement from the width;
//   * no scratch, no allocation, no synchronisation, no workspace: the activations are the caller's buffers.
#include "ft_voc_launch.h"

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
constexpr int MAXD = voc_plan::MAX_DILATION;

template <class C>
__global__ __launch_bounds__(C::THREADS) void resblock_kernel(const float* __restrict__ x, const long* __restrict__ lens, int Tmax,
                                                       int tail, int scale, int ch, int CP, int d, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, const float* __restrict__ w2,
                                                       const float* __restrict__ b2, const float* __restrict__ ws,
                                                       const float* __restrict__ bs, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float smem[voc_plan::lds_floats(voc_plan::RESBLOCK, C::ARR)];
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

// ft_melgan_tile_rows' kinds are the plan's, with the residual block at 2
int plan_kind(int kind) { return kind == 2 ? voc_plan::RESBLOCK : kind >= 0 && kind <= 3 ? kind : -1; }

}  // namespace

extern "C" {

int ft_melgan_tile_rows(int kind, int c) { return voc_plan::tile_rows(plan_kind(kind), c); }

int ft_melgan_conv_in(const float* mel, const long* lens, int B, int n_mels, int Tmax, int tail, float pad_value,
                      const float* w, const float* bias, int cout, float* out, int* err_flag, void* stream) {
  return launch_conv_in<EDGE_REFLECT, true>("melgan_conv_in", mel, lens, B, n_mels, Tmax, tail, pad_value, w, bias, cout, out,
                                            err_flag, stream);
}

int ft_melgan_upsample(const float* x, const long* lens, int B, int Tmax, int tail, int scale, int cin, int cout,
                       int stride, const float* w, const float* bias, float* out, void* stream) {
  return launch_upsample<Act>("melgan_upsample", x, lens, B, Tmax, tail, scale, cin, cout, stride, w, bias, out, stream);
}

int ft_melgan_resblock(const float* x, const long* lens, int B, int Tmax, int tail, int scale, int ch, int dilation,
                       const float* w1, const float* b1, const float* w2, const float* b2, const float* ws,
                       const float* bs, float* out, void* stream) {
  using namespace voc_plan;
  FT_REQUIRE(tile_rows(RESBLOCK, ch) > 0, "melgan_resblock: %d channels must be a multiple of 8 in 8..%d", ch, max_width(RESBLOCK));
  FT_REQUIRE(B >= 1 && Tmax >= 1 && tail >= 0 && scale >= 1 && B <= MAX_BATCH, "melgan_resblock: bad dims");
  FT_REQUIRE(dilation >= 1 && dilation <= MAX_DILATION, "melgan_resblock: dilation %d (1..%d)", dilation, MAX_DILATION);
  FT_REQUIRE((long)((lens ? 1 : Tmax) + tail) * scale > dilation, "melgan_resblock: the shortest item cannot be reflected by %d",
             dilation);
  FT_REQUIRE(x && w1 && b1 && w2 && b2 && ws && bs && out && x != out && aligned16(x), "melgan_resblock: null, aliased or "
             "misaligned pointer");
  const Launch g = residual(RESBLOCK, B, Tmax, tail, scale, ch);
  with_cfg<RESBLOCK>(ch, [&](auto cfg) {
    hipLaunchKernelGGL(resblock_kernel<decltype(cfg)>, grid_of(g), dim3(g.threads), 0, (hipStream_t)stream, x, lens, Tmax, tail,
                       scale, ch, g.cp, dilation, w1, b1, w2, b2, ws, bs, out);
  });
  return ft_check_launch("melgan_resblock");
}

int ft_melgan_conv_out(const float* x, const long* lens, int B, int Tmax, int tail, int scale, int ch, const float* w,
                       float bias, float* wav, short* wav_i16, void* stream) {
  return launch_conv_out<Act, EDGE_REFLECT>("melgan_conv_out", x, lens, B, Tmax, tail, scale, ch, w, bias, wav, wav_i16, stream);
}

}  // extern "C"
