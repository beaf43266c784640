// MelGAN generator for inference on a RAGGED batch of mels (melgan.MelGAN.inference_batch; the definition is DESIGN.md
// section 7, "MelGAN vocoder").  Four kernels: the input convolution, LeakyReLU + transposed convolution in polyphase
// form, the fused residual block, and the output stage.
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
#include <math.h>

#include "ft_common.h"

namespace {

constexpr float SLOPE = 0.2f;

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : SLOPE * v; }

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
template <int RT, bool LRELU>
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
    if (LRELU) {
#pragma unroll
      for (int r = 0; r < RT; ++r) a[r] = make_float4(lrelu(a[r].x), lrelu(a[r].y), lrelu(a[r].z), lrelu(a[r].w));
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

// The arrangement of a workgroup: CMAX the widest input it stages, WR x WC waves (4 or 8), RT row tiles per wave.
template <int CMAX_, int WR_, int WC_, int RT_>
struct Cfg {
  static constexpr int CMAX = CMAX_, WR = WR_, WC = WC_, RT = RT_;
  static constexpr int ROWS = 32 * RT_ * WR_;          // output rows (input rows of the transposed convolution) per tile
  static constexpr int XS = CMAX_ + 4;                 // (the kernels use the runtime width + 4; this sizes the LDS)
  static constexpr int THREADS = 64 * WR_ * WC_;
  static_assert(WR_ * WC_ == 4 || WR_ * WC_ == 8, "four or eight waves");
};

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

// stage rows [first, first + n) of a channels-last item (reflected and clamped against L) into LDS rows 0 .. n - 1
__device__ __forceinline__ void stage_reflected(float* xs, int xrs, const float* __restrict__ item, int C, long first, int n,
                                                long L, int threads) {
  const int c4n = C / 4;
  for (int idx = threadIdx.x; idx < n * c4n; idx += threads) {
    const int i = idx / c4n, c4 = idx - i * c4n;
    const long src = reflect_row(first + i, L);
    *reinterpret_cast<float4*>(xs + i * xrs + 4 * c4) = *reinterpret_cast<const float4*>(item + src * C + 4 * c4);
  }
}

// ---------------------------------------------------------------------------------------------------
// 1. input convolution: out[t][co] = bias[co] + sum over tap, c of W[tap][c][co] x[reflect(t + tap - 3)][c], x[t][c] =
//    (mel[b][c][t] + 5) / 5 for t < len[b] and (pad_value + 5) / 5 for the `tail` appended frames: the normalised mel
//    and the appended frames exist in LDS only.  mel is read as it is, [B, n_mels, Tmax], coalesced along t.
// ---------------------------------------------------------------------------------------------------
template <class C>
__global__ __launch_bounds__(C::THREADS) void conv_in_kernel(const float* __restrict__ mel, const long* __restrict__ lens, int Tmax,
                                                      int tail, float pad_value, int n_mels, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int cout, int CP, float* __restrict__ out,
                                                      int* err) {
  __shared__ __attribute__((aligned(16))) float xs[(C::ROWS + 6) * C::XS];
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
    const long src = reflect_row(t0 - 3 + i, L);
    xs[i * xrs + c] = src < n ? (item[(long)c * Tmax + src] + 5.0f) / 5.0f : padn;
  }
  __syncthreads();
  float* obase = out + ((long)b * (Tmax + tail) + t0) * cout;
  const int row0 = v.wr * 32 * C::RT;
  for (int ct = blockIdx.z * C::WC + v.wc; ct * 32 < cout; ct += C::WC * gridDim.z) {      // grid.z: groups of channel tiles
    const int co = 32 * ct + v.l31;
    f32x16 acc[C::RT];
    fill<C::RT>(acc, bias[co]);
    for (int tap = 0; tap < 7; ++tap)
      mma_panel<C::RT, false>(acc, xs + (row0 + v.l31 + tap) * xrs + 4 * v.hf, xrs,
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
template <class C>
__global__ __launch_bounds__(C::THREADS) void upsample_kernel(const float* __restrict__ x, const long* __restrict__ lens, int Tmax,
                                                       int tail, int scale, int cin, int cout, int CP, int s,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xs[(C::ROWS + 1) * C::XS];
  const int b = blockIdx.y;
  const long q0 = (long)blockIdx.x * C::ROWS;
  const long Lin = item_rows(lens, b, Tmax, tail, scale, nullptr);
  if (q0 > Lin) return;
  const Wave v = Wave::make<C>();
  const int xrs = cin + 4, c4n = cin / 4;
  const float* item = x + (long)b * (Tmax + tail) * scale * cin;
  for (int idx = threadIdx.x; idx < (C::ROWS + 1) * c4n; idx += C::THREADS) {
    const int i = idx / c4n, c4 = idx - i * c4n;
    const long src = q0 - 1 + i;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src >= 0 && src < Lin) val = *reinterpret_cast<const float4*>(item + src * cin + 4 * c4);
    *reinterpret_cast<float4*>(xs + i * xrs + 4 * c4) = val;
  }
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
      mma_panel<C::RT, true>(acc, xs + (row0 + v.l31 + 1) * xrs + 4 * v.hf, xrs, w + ((long)p * cin + 4 * v.hf) * CP + co, CP,
                             cin);
      mma_panel<C::RT, true>(acc, xs + (row0 + v.l31) * xrs + 4 * v.hf, xrs, w + ((long)(p + s) * cin + 4 * v.hf) * CP + co,
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
  stage_reflected(xs, xrs, x + ioff, ch, t0 - d, C::ROWS + 2 * d, L, C::THREADS);
  __syncthreads();
  const int row0 = v.wr * 32 * C::RT;
  for (int ct = v.wc; ct * 32 < ch; ct += C::WC) {
    const int co = 32 * ct + v.l31;
    f32x16 acc[C::RT];
    fill<C::RT>(acc, b1[co]);
    for (int tap = 0; tap < 3; ++tap)
      mma_panel<C::RT, true>(acc, xs + (row0 + v.l31 + tap * d) * xrs + 4 * v.hf, xrs,
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
    mma_panel<C::RT, false>(acc, ms + (row0 + v.l31) * xrs + 4 * v.hf, xrs, w2 + (long)(4 * v.hf) * CP + co, CP, ch);
    mma_panel<C::RT, false>(acc, xs + (row0 + v.l31 + d) * xrs + 4 * v.hf, xrs, ws + (long)(4 * v.hf) * CP + co, CP, ch);
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
// 4. output stage: wav[j] = tanh(bias + sum over tap, c of W[tap][c] lrelu(x[reflect(j + tap - 3)][c])) for j < scale *
//    len[b] (the tail's samples are never formed), exactly 0 behind; wav_i16 = truncate(clamp(32768 wav, -32768, 32767))
//    in the same pass.  One output channel: the MFMA forms P[row][tap] = sum over c of lrelu(x[row][c]) W[c][tap] for the
//    256 staged rows t0 - 3 .. t0 + 252 (taps on the MFMA's N, 7 of 32 columns used: the stage is 0.1 % of the
//    generator's FLOP), P goes to LDS, and sample t0 + o adds P[o + tap][tap] over the taps in ascending order.
//    w: [C][32], column = tap.
// ---------------------------------------------------------------------------------------------------
constexpr int OUT_ROWS = 256, OUT_TILE = OUT_ROWS - 6, OUT_CMAX = 32;

__global__ __launch_bounds__(256) void conv_out_kernel(const float* __restrict__ x, const long* __restrict__ lens, int Tmax,
                                                       int tail, int scale, int ch, const float* __restrict__ w, float bias,
                                                       float* __restrict__ wav, short* __restrict__ wav_i16) {
  typedef Cfg<OUT_CMAX, 4, 1, 2> C;
  __shared__ __attribute__((aligned(16))) float xs[OUT_ROWS * C::XS];
  __shared__ float ps[OUT_ROWS * 8];
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
  stage_reflected(xs, xrs, x + (long)b * (Tmax + tail) * scale * ch, ch, t0 - 3, OUT_ROWS, L, 256);
  __syncthreads();
  const int row0 = v.wr * 32 * C::RT;
  f32x16 acc[C::RT];
  fill<C::RT>(acc, 0.f);
  mma_panel<C::RT, true>(acc, xs + (row0 + v.l31) * xrs + 4 * v.hf, xrs, w + (long)(4 * v.hf) * 32 + v.l31, 32, ch);
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

bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

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
  hipLaunchKernelGGL(conv_in_kernel<In128>, grid, dim3(In128::THREADS), 0, (hipStream_t)stream, mel, lens, Tmax, tail, pad_value, n_mels,
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
  hipLaunchKernelGGL(upsample_kernel<CFG>, grid, dim3(CFG::THREADS), 0, st, x, lens, Tmax, tail, scale, cin, cout, CP, stride, w, bias, out)
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
  hipLaunchKernelGGL(conv_out_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, lens, Tmax, tail, scale, ch, w, bias, wav,
                     wav_i16);
  return ft_check_launch("melgan_conv_out");
}

}  // extern "C"
