// What the vocoder generators share (ft_melgan.hip, ft_hifigan.hip): the per-item row layout, the exact-fp32 MFMA panel
// routine, the workgroup arrangements, the staging of a channels-last tile into LDS under either edge rule, and the
// three kernels both generators run -- the input convolution, LeakyReLU + transposed convolution in polyphase form, and
// the output stage.  The LeakyReLU slope (an Act type) and the edge rule (EDGE_REFLECT / EDGE_ZERO) are template
// parameters; the layout and the rules common to every kernel are stated in the header of ft_melgan.hip.  The arrangements
// themselves, the LDS they need and every limit are ft_voc_plan.h's (host-only); the launchers are in ft_voc_launch.h.
// Everything is a template or __forceinline__, in a named namespace that the two files open with a using-directive.
#pragma once
#include <math.h>

#include "ft_common.h"
#include "ft_voc_plan.h"

namespace ft_voc_tile {

// the activation applied to the A operand on its way from LDS to the MFMA
struct NoAct {
  static constexpr bool ON = false;
  __device__ static __forceinline__ float f(float v) { return v; }
};
struct Lrelu02 {                                 // MelGAN
  static constexpr bool ON = true;
  __device__ static __forceinline__ float f(float v) { return v > 0.f ? v : 0.2f * v; }
};
struct Lrelu01 {                                 // HiFi-GAN
  static constexpr bool ON = true;
  __device__ static __forceinline__ float f(float v) { return v > 0.f ? v : 0.1f * v; }
};
struct Lrelu001 {                                // HiFi-GAN's output stage (torch's default slope)
  static constexpr bool ON = true;
  __device__ static __forceinline__ float f(float v) { return v > 0.f ? v : 0.01f * v; }
};

// what a row outside an item's [0, L) holds
constexpr int EDGE_REFLECT = 0;                  // row -j is row j, row L - 1 + j is row L - 1 - j
constexpr int EDGE_ZERO = 1;                     // zeros

// the row of register e of a 32x32 accumulator tile in lane half hf (the column is the lane's l31)
__device__ __forceinline__ int crow(int e, int hf) { return (e & 3) + 8 * (e >> 2) + 4 * hf; }

// item b's frames (clamped) -> rows at `scale`
__device__ __forceinline__ long item_rows(const long* lens, int b, int Tmax, int tail, int scale, int* err) {
  const long n = lens ? ft_item_len(lens, b, 1, Tmax, err) : (long)Tmax;
  return (n + tail) * scale;
}

// row t of an item of L rows under reflection padding, clamped into the item (a tile's rows at >= L ask for rows that
// one reflection does not bring back; what they compute is never stored)
__device__ __forceinline__ long reflect_row(long t, long L) {
  if (t < 0) t = -t;
  if (t >= L) t = 2 * (L - 1) - t;
  return t < 0 ? 0 : (t >= L ? L - 1 : t);
}

// acc[r] += X[32 r + l31][k] W[k][co], k = 0 .. K - 1 (K % 8 == 0).  xrow: the LDS address of (row l31 of the wave's
// row tile 0, column 4 hf), xrs the row stride in floats; w: the global address of W[4 hf][co of this lane], ldw its row
// stride.  Step (k, i) multiplies feature k + 4 hf + i of row l31 (A) with the same feature's weight (B): one 16-byte LDS
// read per four MFMA steps.
template <int RT, class Act>
__device__ __forceinline__ void mma_panel(f32x16 (&acc)[RT], const float* xrow, int xrs, const float* __restrict__ w,
                                          int ldw, int K) {
  // operands of step k + 8 are fetched before the MFMAs of step k issue: at one or two waves per SIMD nothing else hides
  // the L2 and LDS latencies
  float nb[4];
  float4 na[RT];
#pragma unroll
  for (int i = 0; i < 4; ++i) nb[i] = w[i * ldw];
#pragma unroll
  for (int r = 0; r < RT; ++r) na[r] = *reinterpret_cast<const float4*>(xrow + 32 * r * xrs);
  for (int k = 0; k < K; k += 8) {
    const float b0 = nb[0], b1 = nb[1], b2 = nb[2], b3 = nb[3];
    float4 a[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) a[r] = na[r];
    if (k + 8 < K) {
      const float* wk = w + (long)(k + 8) * ldw;
#pragma unroll
      for (int i = 0; i < 4; ++i) nb[i] = wk[i * ldw];
#pragma unroll
      for (int r = 0; r < RT; ++r) na[r] = *reinterpret_cast<const float4*>(xrow + 32 * r * xrs + k + 8);
    }
    if (Act::ON) {
#pragma unroll
      for (int r = 0; r < RT; ++r) a[r] = make_float4(Act::f(a[r].x), Act::f(a[r].y), Act::f(a[r].z), Act::f(a[r].w));
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r].x, b0, acc[r], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r].y, b1, acc[r], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r].z, b2, acc[r], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r].w, b3, acc[r], 0, 0, 0);
  }
}

template <int RT>
__device__ __forceinline__ void fill(f32x16 (&acc)[RT], float v) {
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[r][e] = v;
}

// The arrangement of a workgroup as a type: voc_plan::Arr's CMAX the widest input it stages, WR x WC waves (4 or 8), RT
// row tiles per wave.  PlanCfg<kind, i> is arrangement i of the plan's table for a kind; no other Cfg is instantiated.
template <int CMAX_, int WR_, int WC_, int RT_>
struct Cfg {
  static constexpr voc_plan::Arr ARR = {CMAX_, WR_, WC_, RT_};
  static constexpr int CMAX = CMAX_, WR = WR_, WC = WC_, RT = RT_;
  static constexpr int ROWS = ARR.rows();              // output rows (input rows of the transposed convolution) per tile
  static constexpr int XS = ARR.xs();                  // (the kernels use the runtime width + 4; this sizes the LDS)
  static constexpr int THREADS = ARR.threads();
};
template <int KIND, int I>
using PlanCfg = Cfg<voc_plan::arr(KIND, I).cmax, voc_plan::arr(KIND, I).wr, voc_plan::arr(KIND, I).wc, voc_plan::arr(KIND, I).rt>;

struct Wave {
  int lane, l31, hf, wr, wc;
  template <class C>
  __device__ static Wave make() {
    Wave v;
    const int wave = threadIdx.x >> 6;
    v.lane = threadIdx.x & 63;
    v.l31 = v.lane & 31;
    v.hf = v.lane >> 5;
    v.wr = wave / C::WC;
    v.wc = wave % C::WC;
    return v;
  }
};

// stage rows [first, first + n) of a channels-last item of L rows into LDS rows 0 .. n - 1: reflected and clamped
// against L (EDGE_REFLECT), or zeros outside [0, L) (EDGE_ZERO).  No row at >= L is loaded under either rule.
template <int EDGE>
__device__ __forceinline__ void stage_rows(float* xs, int xrs, const float* __restrict__ item, int C, long first, int n, long L,
                                           int threads) {
  const int c4n = C / 4;
  for (int idx = threadIdx.x; idx < n * c4n; idx += threads) {
    const int i = idx / c4n, c4 = idx - i * c4n;
    if (EDGE == EDGE_REFLECT) {
      const long src = reflect_row(first + i, L);
      *reinterpret_cast<float4*>(xs + i * xrs + 4 * c4) = *reinterpret_cast<const float4*>(item + src * C + 4 * c4);
    } else {
      const long src = first + i;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (src >= 0 && src < L) val = *reinterpret_cast<const float4*>(item + src * C + 4 * c4);
      *reinterpret_cast<float4*>(xs + i * xrs + 4 * c4) = val;
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// 1. input convolution: out[t][co] = bias[co] + sum over tap, c of W[tap][c][co] x[edge(t + tap - 3)][c].  mel is read
//    as it is, [B, n_mels, Tmax], coalesced along t.
//    NORM (MelGAN): x[t][c] = (mel[b][c][t] + 5) / 5 for t < len[b] and (pad_value + 5) / 5 for the `tail` appended
//    frames: the normalised mel and the appended frames exist in LDS only.  !NORM (HiFi-GAN): x = mel, tail = 0.
// ---------------------------------------------------------------------------------------------------
template <class C, int EDGE, bool NORM>
__global__ __launch_bounds__(C::THREADS) void conv_in_kernel(const float* __restrict__ mel, const long* __restrict__ lens, int Tmax,
                                                      int tail, float pad_value, int n_mels, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int cout, int CP, float* __restrict__ out,
                                                      int* err) {
  __shared__ __attribute__((aligned(16))) float xs[voc_plan::lds_floats(voc_plan::CONV_IN, C::ARR)];
  const int b = blockIdx.y;
  const long t0 = (long)blockIdx.x * C::ROWS;
  const long n = item_rows(lens, b, Tmax, 0, 1, (blockIdx.x == 0 && threadIdx.x == 0) ? err : nullptr);
  const long L = n + tail;
  if (t0 >= L) return;
  const Wave v = Wave::make<C>();
  const int xrs = n_mels + 4;
  const float* item = mel + (long)b * n_mels * Tmax;
  const float padn = (pad_value + 5.0f) / 5.0f;
  constexpr int NR = C::ROWS + 6;
  for (int idx = threadIdx.x; idx < NR * n_mels; idx += C::THREADS) {
    const int c = idx / NR, i = idx - c * NR;
    if (EDGE == EDGE_REFLECT) {
      const long src = reflect_row(t0 - 3 + i, L);
      if (NORM) xs[i * xrs + c] = src < n ? (item[(long)c * Tmax + src] + 5.0f) / 5.0f : padn;
      else xs[i * xrs + c] = src < n ? item[(long)c * Tmax + src] : pad_value;
    } else {
      const long src = t0 - 3 + i;
      float val = 0.f;                                    // (the zero edge pads the convolution's input, after NORM)
      if (src >= 0 && src < n) val = NORM ? (item[(long)c * Tmax + src] + 5.0f) / 5.0f : item[(long)c * Tmax + src];
      else if (src >= n && src < L) val = NORM ? padn : pad_value;
      xs[i * xrs + c] = val;
    }
  }
  __syncthreads();
  float* obase = out + ((long)b * (Tmax + tail) + t0) * cout;
  const int row0 = v.wr * 32 * C::RT;
  for (int ct = blockIdx.z * C::WC + v.wc; ct * 32 < cout; ct += C::WC * gridDim.z) {      // grid.z: groups of channel tiles
    const int co = 32 * ct + v.l31;
    f32x16 acc[C::RT];
    fill<C::RT>(acc, bias[co]);
    for (int tap = 0; tap < 7; ++tap)
      mma_panel<C::RT, NoAct>(acc, xs + (row0 + v.l31 + tap) * xrs + 4 * v.hf, xrs,
                              w + ((long)tap * n_mels + 4 * v.hf) * CP + co, CP, n_mels);
    if (co < cout) {
#pragma unroll
      for (int r = 0; r < C::RT; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = row0 + 32 * r + crow(e, v.hf);
          if (t0 + row < L) obase[(long)row * cout + co] = acc[r][e];
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// 2. LeakyReLU + ConvTranspose1d(k = 2 s, stride s, padding s / 2) in polyphase form.  Output row j = s q + p - s / 2
//    takes exactly two input rows: q with kernel tap p and q - 1 with tap p + s (rows -1 and Lin are zero): per phase p
//    one [rows, 2 Cin] x [2 Cin, Cout] product over the same staged input rows.  A tile is C::ROWS values of q (q = 0 ..
//    Lin inclusive: q = Lin still feeds the phases p < s / 2); LDS row i holds input row q0 - 1 + i.  No zero-stuffed
//    input, no scatter.  w: [2 s][Cin][CP], tap-major.
// ---------------------------------------------------------------------------------------------------
template <class C, class Act>
__global__ __launch_bounds__(C::THREADS) void upsample_kernel(const float* __restrict__ x, const long* __restrict__ lens, int Tmax,
                                                       int tail, int scale, int cin, int cout, int CP, int s,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xs[voc_plan::lds_floats(voc_plan::UPSAMPLE, C::ARR)];
  const int b = blockIdx.y;
  const long q0 = (long)blockIdx.x * C::ROWS;
  const long Lin = item_rows(lens, b, Tmax, tail, scale, nullptr);
  if (q0 > Lin) return;
  const Wave v = Wave::make<C>();
  const int xrs = cin + 4;
  stage_rows<EDGE_ZERO>(xs, xrs, x + (long)b * (Tmax + tail) * scale * cin, cin, q0 - 1, C::ROWS + 1, Lin, C::THREADS);
  __syncthreads();
  const long Lout = Lin * s;
  float* obase = out + (long)b * (Tmax + tail) * scale * s * cout;
  const int row0 = v.wr * 32 * C::RT;
  for (int ct = v.wc; ct * 32 < cout; ct += C::WC) {
    const int co = 32 * ct + v.l31;
    const float bco = bias[co];
    for (int p = blockIdx.z; p < s; p += gridDim.z) {      // grid.z: 1, or one phase per workgroup
      f32x16 acc[C::RT];
      fill<C::RT>(acc, bco);
      // input row q is LDS row q - q0 + 1, row q - 1 is LDS row q - q0
      mma_panel<C::RT, Act>(acc, xs + (row0 + v.l31 + 1) * xrs + 4 * v.hf, xrs, w + ((long)p * cin + 4 * v.hf) * CP + co, CP,
                            cin);
      mma_panel<C::RT, Act>(acc, xs + (row0 + v.l31) * xrs + 4 * v.hf, xrs, w + ((long)(p + s) * cin + 4 * v.hf) * CP + co,
                            CP, cin);
      if (co < cout) {
#pragma unroll
        for (int r = 0; r < C::RT; ++r)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const long j = (q0 + row0 + 32 * r + crow(e, v.hf)) * s + p - s / 2;
            if (j >= 0 && j < Lout) obase[j * cout + co] = acc[r][e];
          }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// 4. output stage: wav[j] = tanh(bias + sum over tap, c of W[tap][c] lrelu(x[edge(j + tap - 3)][c])) for j < scale *
//    len[b] (the tail's samples are never formed), exactly 0 behind; wav_i16 = truncate(clamp(32768 wav, -32768, 32767))
//    in the same pass.  One output channel: the MFMA forms P[row][tap] = sum over c of lrelu(x[row][c]) W[c][tap] for the
//    256 staged rows t0 - 3 .. t0 + 252 (taps on the MFMA's N, 7 of 32 columns used: the stage is 0.1 % of the
//    generator's FLOP), P goes to LDS, and sample t0 + o adds P[o + tap][tap] over the taps in ascending order.
//    w: [C][32], column = tap.
// ---------------------------------------------------------------------------------------------------
using voc_plan::OUT_ROWS;
using voc_plan::OUT_TILE;
typedef PlanCfg<voc_plan::CONV_OUT, 0> OutCfg;

template <class Act, int EDGE>
__global__ __launch_bounds__(OutCfg::THREADS) void conv_out_kernel(const float* __restrict__ x, const long* __restrict__ lens, int Tmax,
                                                       int tail, int scale, int ch, const float* __restrict__ w, float bias,
                                                       float* __restrict__ wav, short* __restrict__ wav_i16) {
  typedef OutCfg C;
  __shared__ __attribute__((aligned(16))) float xs[OUT_ROWS * C::XS];
  __shared__ float ps[OUT_ROWS * 8];
  static_assert(sizeof(xs) + sizeof(ps) == voc_plan::lds_bytes(voc_plan::CONV_OUT, C::ARR), "the plan's bytes");
  const int b = blockIdx.y;
  const long t0 = (long)blockIdx.x * OUT_TILE;
  const long nout = item_rows(lens, b, Tmax, 0, scale, nullptr);
  const long L = nout + (long)tail * scale;
  const long ld = (long)Tmax * scale;
  const long j = t0 + threadIdx.x;
  const bool mine = threadIdx.x < OUT_TILE && j < ld;
  if (t0 >= nout) {
    if (mine) {
      wav[b * ld + j] = 0.f;
      wav_i16[b * ld + j] = 0;
    }
    return;
  }
  const Wave v = Wave::make<C>();
  const int xrs = ch + 4;
  stage_rows<EDGE>(xs, xrs, x + (long)b * (Tmax + tail) * scale * ch, ch, t0 - 3, OUT_ROWS, L, 256);
  __syncthreads();
  const int row0 = v.wr * 32 * C::RT;
  f32x16 acc[C::RT];
  fill<C::RT>(acc, 0.f);
  mma_panel<C::RT, Act>(acc, xs + (row0 + v.l31) * xrs + 4 * v.hf, xrs, w + (long)(4 * v.hf) * 32 + v.l31, 32, ch);
  if (v.l31 < 7) {
#pragma unroll
    for (int r = 0; r < C::RT; ++r)
#pragma unroll
      for (int e = 0; e < 16; ++e) ps[(row0 + 32 * r + crow(e, v.hf)) * 8 + v.l31] = acc[r][e];
  }
  __syncthreads();
  if (!mine) return;
  float y = 0.f, q = 0.f;
  if (j < nout) {
    float sum = bias;
#pragma unroll
    for (int tap = 0; tap < 7; ++tap) sum += ps[(threadIdx.x + tap) * 8 + tap];
    y = tanhf(sum);
    q = fminf(fmaxf(y * 32768.0f, -32768.0f), 32767.0f);
  }
  wav[b * ld + j] = y;
  wav_i16[b * ld + j] = (short)(int)q;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace ft_voc_tile
