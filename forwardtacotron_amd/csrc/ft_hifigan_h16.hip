// HiFi-GAN's residual convolution with fp16 MATRIX OPERANDS (hifigan.HiFiGAN.matmul_dtype = 'fp16'; the mode's arithmetic is
// DESIGN.md section 7, "HiFi-GAN vocoder", fp16 mode).  out = acc_rule(res + bias + conv_{k, d}(lrelu_0.1(x))) as
// ft_hifigan.hip's resconv_kernel, with
//   a   = fp16_rne(clamp(lrelu_0.1(x), -65504, 65504)), formed ONCE while the tile is staged into LDS (NaN stays NaN, a
//         finite x never becomes Inf, the zero rows outside [0, L) stay exact zeros),
//   w_h = fp16_rne(folded weight), packed on the host side (hifigan.pack_taps_h16),
// products exact and accumulation in fp32 inside v_mfma_f32_32x32x16_f16, starting from the fp32 bias, in an order that is
// a function of the width, the taps and the dilation alone; the residual is added in fp32 FROM MEMORY (the tile no longer
// holds raw x); activations stay fp32 in HBM.  The contract is resconv_kernel's: grid = (tiles of one item, B), a workgroup
// wholly past L leaves, no row at t >= L is loaded or stored, no scratch, no workspace, no atomics.  ft_hifigan.hip and
// the kernels of ft_voc_tile.h are not touched by this file: fp32 mode launches what it always launched.
//
// Operands.  Lane l of a wave (l31 = l & 31, hf = l >> 5) gives the MFMA A[row l31][k = 8 hf + j] and B[k = 8 hf + j][col
// l31], j = 0..7: 16 bytes each.  A is one ds_read_b128 at LDS row (row + tap d), halves 16 s + 8 hf ..; the row stride
// cpad + 8 halves keeps the reads conflict-free (ft_voc_plan_h16.h).  B is one 16-byte global load: the pack is
// [k taps][cpad / 8][CP columns][8 halves], so chunk (tap, 2 s + hf) of column co is at ((tap cpad / 8 + 2 s + hf) CP + co)
// and the 32 lanes of a half-wave read 512 consecutive bytes.  The width is padded to cpad, a multiple of 16, with zeros in
// the tile and in the pack; zeros contribute exactly 0.
#include "ft_voc_launch.h"
#include "ft_voc_plan_h16.h"

namespace {

using namespace ft_voc_tile;

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// lrelu_0.1, the saturating clamp (comparisons, so NaN passes through) and the round-to-nearest-even conversion
__device__ __forceinline__ _Float16 operand(float v) {
  v = Lrelu01::f(v);
  v = v > 65504.f ? 65504.f : v;
  v = v < -65504.f ? -65504.f : v;
  return (_Float16)v;
}

// rows [first, first + n) of a channels-last fp32 item of L rows -> LDS rows 0 .. n - 1 as fp16 operands, cpad halves
// each: zeros outside [0, L) and behind the width C.  No row at >= L is loaded.
__device__ __forceinline__ void stage_rows_h16(_Float16* xs, int xrs, const float* __restrict__ item, int C, int cpad, long first,
                                               int n, long L, int threads) {
  const int c8n = cpad / 8;
  for (int idx = threadIdx.x; idx < n * c8n; idx += threads) {
    const int i = idx / c8n, c8 = idx - i * c8n;
    const long src = first + i;
    h16x8 val = {0, 0, 0, 0, 0, 0, 0, 0};
    if (src >= 0 && src < L && 8 * c8 < C) {
      const float4 lo = *reinterpret_cast<const float4*>(item + src * C + 8 * c8);
      const float4 hi = *reinterpret_cast<const float4*>(item + src * C + 8 * c8 + 4);
      val[0] = operand(lo.x), val[1] = operand(lo.y), val[2] = operand(lo.z), val[3] = operand(lo.w);
      val[4] = operand(hi.x), val[5] = operand(hi.y), val[6] = operand(hi.z), val[7] = operand(hi.w);
    }
    *reinterpret_cast<h16x8*>(xs + i * xrs + 8 * c8) = val;
  }
}

constexpr int WDEPTH = 4;                        // steps of weights in flight ahead of the MFMAs

template <int I>
using H16Cfg = Cfg<voc_plan_h16::ARRS[I].cmax, voc_plan_h16::ARRS[I].wr, voc_plan_h16::ARRS[I].wc, voc_plan_h16::ARRS[I].rt>;

// res: nullptr, or what is added to the value from memory (the launcher passes x itself for res_mode 1)
template <class C>
__global__ __launch_bounds__(C::THREADS) void resconv_h16_kernel(const float* __restrict__ x, const long* __restrict__ lens,
                                                          int Tmax, int scale, int ch, int CP, int k, int d,
                                                          const h16x8* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ res, int acc_mode, float nk,
                                                          float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) _Float16 xs[voc_plan_h16::lds_halves(C::ARR)];
  const int b = blockIdx.y;
  const long t0 = (long)blockIdx.x * C::ROWS;
  const long L = item_rows(lens, b, Tmax, 0, scale, nullptr);
  if (t0 >= L) return;
  const Wave v = Wave::make<C>();
  const int cpad = voc_plan_h16::cpad(ch), xrs = voc_plan_h16::row_halves(cpad), halo = d * (k - 1) / 2;
  const long ioff = (long)b * Tmax * scale * ch;
  stage_rows_h16(xs, xrs, x + ioff, ch, cpad, t0 - halo, C::ROWS + 2 * halo, L, C::THREADS);
  __syncthreads();
  const int row0 = v.wr * 32 * C::RT;
  const int KS = cpad / voc_plan_h16::KSTEP, steps = k * KS;
  const _Float16* xa = xs + (row0 + v.l31) * xrs + 8 * v.hf;
  for (int ct = v.wc; ct * 32 < ch; ct += C::WC) {
    const int co = 32 * ct + v.l31;
    f32x16 acc[C::RT];
    fill<C::RT>(acc, bias[co]);
    // step s = tap KS + ks multiplies features 16 ks + 8 hf + j of LDS row (row + tap d) with chunk 2 s + hf of the pack.
    // The weights of the next WDEPTH steps are in flight while the MFMAs of the current WDEPTH steps issue (an L2 hit is
    // several hundred cycles, a step's MFMAs 32 RT, and there are one or two waves per SIMD); the LDS operands are
    // fetched one step ahead.  The order of the steps, and with it every sum, does not depend on WDEPTH.
    const h16x8* wl = w + (long)v.hf * CP + co;
    const h16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    h16x8 cur[WDEPTH], nxt[WDEPTH];
#pragma unroll
    for (int i = 0; i < WDEPTH; ++i) cur[i] = i < steps ? wl[(long)2 * i * CP] : zero;
    h16x8 na[C::RT];
#pragma unroll
    for (int r = 0; r < C::RT; ++r) na[r] = *reinterpret_cast<const h16x8*>(xa + 32 * r * xrs);
    int ks = 0, rowoff = 0;                        // of the NEXT step: its 16-block, tap d xrs
    for (int s0 = 0; s0 < steps; s0 += WDEPTH) {
#pragma unroll
      for (int i = 0; i < WDEPTH; ++i) nxt[i] = s0 + WDEPTH + i < steps ? wl[(long)2 * (s0 + WDEPTH + i) * CP] : zero;
#pragma unroll
      for (int i = 0; i < WDEPTH; ++i) {
        if (s0 + i < steps) {
          h16x8 a[C::RT];
#pragma unroll
          for (int r = 0; r < C::RT; ++r) a[r] = na[r];
          if (++ks == KS) {
            ks = 0;
            rowoff += d * xrs;
          }
          if (s0 + i + 1 < steps) {
#pragma unroll
            for (int r = 0; r < C::RT; ++r) na[r] = *reinterpret_cast<const h16x8*>(xa + 32 * r * xrs + rowoff + 16 * ks);
          }
#pragma unroll
          for (int r = 0; r < C::RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[r], cur[i], acc[r], 0, 0, 0);
        }
      }
#pragma unroll
      for (int i = 0; i < WDEPTH; ++i) cur[i] = nxt[i];
    }
    if (co < ch) {
#pragma unroll
      for (int r = 0; r < C::RT; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = row0 + 32 * r + crow(e, v.hf);
          if (t0 + row < L) {
            const long at = ioff + (t0 + row) * ch + co;
            float val = acc[r][e];
            if (res) val += res[at];
            if (acc_mode >= 1) val = out[at] + val;
            if (acc_mode == 2) val = val / nk;
            out[at] = val;
          }
        }
    }
  }
}

template <class F, int... I>
void with_h16_cfg_at(int i, F& f, std::integer_sequence<int, I...>) {
  (void)((i == I && (f(H16Cfg<I>()), true)) || ...);
}

}  // namespace

extern "C" {

int ft_hifigan_h16_plan(int field, int c) { return voc_plan_h16::query(field, c); }

int ft_hifigan_resconv_h16(const float* x, const long* lens, int B, int Tmax, int scale, int ch, int k, int dilation,
                           const void* w, const float* bias, const float* res, int res_mode, int acc_mode, int nk, float* out,
                           void* stream) {
  using namespace voc_plan;
  FT_REQUIRE(voc_plan_h16::tile_rows(ch) > 0, "hifigan_resconv_h16: %d channels must be a multiple of 8 in 8..%d", ch,
             voc_plan_h16::MAX_WIDTH);
  FT_REQUIRE(B >= 1 && Tmax >= 1 && scale >= 1 && B <= MAX_BATCH, "hifigan_resconv_h16: bad dims");
  FT_REQUIRE(taps_ok(k, 1), "hifigan_resconv_h16: %d taps (odd, 1..%d)", k, MAX_TAPS);
  FT_REQUIRE(dilation >= 1 && halo(k, dilation) <= MAX_HALO,
             "hifigan_resconv_h16: dilation %d with %d taps needs a halo of %d rows (at most %d)", dilation, k, halo(k, dilation),
             MAX_HALO);
  FT_REQUIRE(res_mode >= 0 && res_mode <= 2 && (res_mode != 2 || res) && acc_mode >= 0 && acc_mode <= 2 && nk >= 1,
             "hifigan_resconv_h16: bad res_mode / acc_mode / nk");
  FT_REQUIRE(x && w && bias && out && x != out && aligned16(x) && aligned16(w),
             "hifigan_resconv_h16: null, aliased or misaligned pointer");
  const float* add = res_mode == 1 ? x : res_mode == 2 ? res : nullptr;      // the tile holds fp16 lrelu(x): raw x is read again
  const Launch g = voc_plan_h16::launch(B, Tmax, scale, ch);
  auto go = [&](auto cfg) {
    hipLaunchKernelGGL(resconv_h16_kernel<decltype(cfg)>, grid_of(g), dim3(g.threads), 0, (hipStream_t)stream, x, lens, Tmax,
                       scale, ch, g.cp, k, dilation, (const h16x8*)w, bias, add, acc_mode, (float)nk, out);
  };
  with_h16_cfg_at(voc_plan_h16::pick(ch), go, std::make_integer_sequence<int, voc_plan_h16::COUNT>());
  return ft_check_launch("hifigan_resconv_h16");
}

}  // extern "C"
