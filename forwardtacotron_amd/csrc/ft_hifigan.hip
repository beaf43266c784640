// HiFi-GAN generator for inference on a RAGGED batch of mels (hifigan.HiFiGAN.inference_batch; the definition is
// DESIGN.md section 7, "HiFi-GAN vocoder").  The layout and the rules are those of ft_melgan.hip's header, with tail = 0
// and ZERO edges in place of reflection: channels-last rows, item b at stride Tmax * scale with its own L = len[b] * scale
// read on the device, grid = (tiles of one item, B), workgroups wholly past L leave, rows past L are neither loaded nor
// stored, the zero rows outside [0, L) are resolved while a tile is staged into LDS, every product runs through
// mma_panel in a k order that is a function of the widths and taps alone, no scratch, no workspace, no atomics.
//
// The input convolution, the transposed convolution and the output stage are the kernels of ft_voc_tile.h at HiFi-GAN's
// parameters (no normalisation, slope 0.1 / 0.01, zero edges), launched through ft_voc_launch.h.  This file's own are the
// residual convolution and the fused pair of ResBlock1.  Arrangements, LDS bytes, limits and grids: ft_voc_plan.h.
#include "ft_voc_launch.h"

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
template <class C>
__global__ __launch_bounds__(C::THREADS) void resconv_kernel(const float* __restrict__ x, const long* __restrict__ lens, int Tmax,
                                                      int scale, int ch, int CP, int k, int d, const float* __restrict__ w,
                                                      const float* __restrict__ bias, const float* __restrict__ res,
                                                      int res_mode, int acc_mode, float nk, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xs[voc_plan::lds_floats(voc_plan::RESCONV, C::ARR)];
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
constexpr int PAIR_H1 = voc_plan::PAIR_HALO;       // d (k - 1) / 2 of the first convolution

template <class C>
__global__ __launch_bounds__(C::THREADS) void respair_kernel(const float* __restrict__ x, const long* __restrict__ lens, int Tmax,
                                                      int scale, int ch, int CP, int k, int d, const float* __restrict__ w1,
                                                      const float* __restrict__ b1, const float* __restrict__ w2,
                                                      const float* __restrict__ b2, int acc_mode, float nk,
                                                      float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float smem[voc_plan::lds_floats(voc_plan::RESPAIR, C::ARR)];
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

}  // namespace

extern "C" {

int ft_hifigan_tile_rows(int kind, int c) { return kind >= 0 && kind <= 4 ? voc_plan::tile_rows(kind, c) : 0; }

// the plan's limits and decisions for the Python side (hip.HIFIGAN_*, hifigan.pair_is_fused): host-only
int ft_voc_plan(int field, int a, int b, int c) { return voc_plan::query(field, a, b, c); }

int ft_hifigan_conv_in(const float* mel, const long* lens, int B, int n_mels, int Tmax, const float* w, const float* bias,
                       int cout, float* out, int* err_flag, void* stream) {
  return launch_conv_in<EDGE_ZERO, false>("hifigan_conv_in", mel, lens, B, n_mels, Tmax, 0, 0.f, w, bias, cout, out, err_flag,
                                          stream);
}

int ft_hifigan_upsample(const float* x, const long* lens, int B, int Tmax, int scale, int cin, int cout, int stride,
                        const float* w, const float* bias, float* out, void* stream) {
  return launch_upsample<Act>("hifigan_upsample", x, lens, B, Tmax, 0, scale, cin, cout, stride, w, bias, out, stream);
}

int ft_hifigan_resconv(const float* x, const long* lens, int B, int Tmax, int scale, int ch, int k, int dilation,
                       const float* w, const float* bias, const float* res, int res_mode, int acc_mode, int nk, float* out,
                       void* stream) {
  using namespace voc_plan;
  FT_REQUIRE(tile_rows(RESCONV, ch) > 0, "hifigan_resconv: %d channels must be a multiple of 8 in 8..%d", ch, max_width(RESCONV));
  FT_REQUIRE(B >= 1 && Tmax >= 1 && scale >= 1 && B <= MAX_BATCH, "hifigan_resconv: bad dims");
  FT_REQUIRE(taps_ok(k, 1), "hifigan_resconv: %d taps (odd, 1..%d)", k, MAX_TAPS);
  FT_REQUIRE(dilation >= 1 && halo(k, dilation) <= MAX_HALO, "hifigan_resconv: dilation %d with %d taps needs a halo of %d rows (at most %d)",
             dilation, k, halo(k, dilation), MAX_HALO);
  FT_REQUIRE(res_mode >= 0 && res_mode <= 2 && (res_mode != 2 || res) && acc_mode >= 0 && acc_mode <= 2 && nk >= 1,
             "hifigan_resconv: bad res_mode / acc_mode / nk");
  FT_REQUIRE(x && w && bias && out && x != out && aligned16(x), "hifigan_resconv: null, aliased or misaligned pointer");
  const Launch g = residual(RESCONV, B, Tmax, 0, scale, ch);
  with_cfg<RESCONV>(ch, [&](auto cfg) {
    hipLaunchKernelGGL(resconv_kernel<decltype(cfg)>, grid_of(g), dim3(g.threads), 0, (hipStream_t)stream, x, lens, Tmax, scale,
                       ch, g.cp, k, dilation, w, bias, res, res_mode, acc_mode, (float)nk, out);
  });
  return ft_check_launch("hifigan_resconv");
}

int ft_hifigan_respair(const float* x, const long* lens, int B, int Tmax, int scale, int ch, int k, int dilation,
                       const float* w1, const float* b1, const float* w2, const float* b2, int acc_mode, int nk, float* out,
                       void* stream) {
  using namespace voc_plan;
  FT_REQUIRE(tile_rows(RESPAIR, ch) > 0, "hifigan_respair: %d channels must be a multiple of 8 in 8..%d (wider pairs run as two launches)",
             ch, max_width(RESPAIR));
  FT_REQUIRE(B >= 1 && Tmax >= 1 && scale >= 1 && B <= MAX_BATCH, "hifigan_respair: bad dims");
  FT_REQUIRE(taps_ok(k, 3), "hifigan_respair: %d taps (odd, 3..%d)", k, MAX_TAPS);
  FT_REQUIRE(dilation >= 1 && halo(k, dilation) <= PAIR_HALO, "hifigan_respair: dilation %d with %d taps needs a halo of %d rows (at most %d)",
             dilation, k, halo(k, dilation), PAIR_HALO);
  FT_REQUIRE(acc_mode >= 0 && acc_mode <= 2 && nk >= 1, "hifigan_respair: bad acc_mode / nk");
  FT_REQUIRE(x && w1 && b1 && w2 && b2 && out && x != out && aligned16(x), "hifigan_respair: null, aliased or misaligned pointer");
  const Launch g = respair(B, Tmax, scale, ch, k);
  with_cfg<RESPAIR>(ch, [&](auto cfg) {
    hipLaunchKernelGGL(respair_kernel<decltype(cfg)>, grid_of(g), dim3(g.threads), 0, (hipStream_t)stream, x, lens, Tmax, scale,
                       ch, g.cp, k, dilation, w1, b1, w2, b2, acc_mode, (float)nk, out);
  });
  return ft_check_launch("hifigan_respair");
}

int ft_hifigan_conv_out(const float* x, const long* lens, int B, int Tmax, int scale, int ch, const float* w, float bias,
                        float* wav, short* wav_i16, void* stream) {
  return launch_conv_out<Lrelu001, EDGE_ZERO>("hifigan_conv_out", x, lens, B, Tmax, 0, scale, ch, w, bias, wav, wav_i16, stream);
}

}  // extern "C"
