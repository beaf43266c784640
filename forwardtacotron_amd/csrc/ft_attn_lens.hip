// Length-aware fused self-attention for inference on a RAGGED batch (FastPitch.generate_batch): att = softmax(scale Q K^T
// over the item's own keys) V between the in- and the out-projection, with the item lengths read on the device.
//   item b, L = min(max(lens[b], 0), T):  rows t < L of att hold the attention over keys < L, rows t >= L hold exactly 0.
// What lies past an item's length costs nothing and cannot leak: a workgroup whose 128 queries are all at t >= L stores
// its zeros and leaves, every other workgroup's key loop ends at ceil(L / 64) blocks, and every load of a qkv row is
// guarded on L (rows at t >= L arrive as zeros in registers -- a NaN in the padding never meets a multiplication).
// No dropout, no log-sum-exp, no byte mask: the training kernels are in ft_attn.hip.
//
// Both precisions keep the orientation of ft_attn_fwd_kernel (score tile transposed, X = K Q^T [32 keys x 32 queries], query
// on the lane, online softmax in-lane plus one exchange between the lane halves, O^T += V^T P) and share its online-softmax
// code; workgroup = 4 waves = 128 queries of one (item, head), keys in blocks of 64, next block's global loads in flight
// during the current block's MFMAs.
//   bf16 = 1: the arithmetic of ft_attn_fwd_kernel, instruction for instruction (operands rounded to bf16 while staged,
//     v_mfma_f32_32x32x16_bf16, same key permutation and block order, the tile helpers of ft_attn_tile.h): valid rows
//     are bit-equal to ft_attn_fwd with the byte mask t >= L at p_drop = 0 -- a fully masked key block there leaves m, l
//     and o unchanged, a masked key inside a block contributes p = 0 either way.
//   bf16 = 0: fp32-exact products on the fp32-input MFMA v_mfma_f32_32x32x2_f32 (same C/D layout, so the same softmax
//     code).  K and V tiles are fp32 row-major in LDS.  X: lane (key or query l31, half hf) covers the features
//     8 j + 4 hf + i of its row (one 16-byte read per four MFMA steps; A from the K tile, B = the query's registers).
//     O^T += V^T P: register e of the probability tile holds key crow(e, hf) for query l31 -- as it stands the B operand of
//     one 32x32x2 step over the keys crow(e, 0), crow(e, 1); the A operand V[crow(e, hf)][32 dt + l31] is a plain read of
//     consecutive floats of one V row per lane half: no shuffle, no transposing read.
//     Row strides: K rows HD + 4 floats (16 lanes x 16 bytes of a b128 read phase tile the 64 banks), V rows HD + 8 floats
//     (the two lane halves read rows 4 apart: 4 * (HD + 8) = 32 mod 64 banks, so they do not meet).
//     LDS: hd = 128: 33.0 + 34.0 KB, one workgroup of 4 waves per CU pair of tiles, 1 wave per SIMD (the 512-register
//     budget holds q (64) + o (64) + x (32) + the 64 prefetch registers); hd = 64: 17.0 + 18.0 KB, 2 waves per SIMD.
//     Bound: the MFMA pipe -- 32x32x2 issues every 64 cycles, 384 of them per wave and 64-key block at hd = 128 (1/16 of
//     the bf16 rate); the T = 840 frame-side layer is 23 GFLOP of the chip's ~157 TF fp32 MFMA peak.
//
// Head widths 192 and 256 (the multispeaker models: 384 / 2 heads in the predictors, 512 / 2 heads in the trunk) do not fit
// that layout -- fp32 q and o alone would be 256 registers per lane at hd = 256, the 64-key K + V tiles 134 KB.  They run in
// the *_wide_* kernels below, same orientation and same online softmax, with another split of the work:
//   keys in blocks of 32 (one score tile), workgroup = 4 waves = TWO PAIRS of waves, 64 queries; the two waves of a pair
//   share the pair's 32 queries and split the HEAD WIDTH: wave `half` holds features [half hd/2, (half + 1) hd/2) of its
//   queries, forms the PARTIAL score tile over those features, and owns those columns of O.  The two partial tiles are
//   summed through LDS (one 4 KB tile per wave; x = own + other, which is the same fp32 sum in both waves because the
//   addition commutes), so both waves of a pair carry identical m, l and probabilities, and no product is formed twice.
//   Per 32-key block: stage K and V, barrier, partial X, exchange, barrier, softmax, O^T += V^T P over the wave's columns.
//   Budget per lane / workgroup (hd = 256; 192 in brackets), as the compiler reports it in DESIGN.md section 7:
//     fp32: q 64 (48) + o 64 (48) + x 16 + K and V prefetch 64 (48) registers; LDS 32 x (hd + 4) + 32 x (hd + 8) floats +
//       16 KB exchange = 83,456 B (67,072 B): one workgroup per CU, 1 wave per SIMD -- the LDS, not the register file,
//       sets the occupancy (the compiler takes 256 VGPRs + 140 (58) AGPRs, no scratch).  Ceiling: the 32x32x2 MFMA pipe like
//       the narrow kernel (hd / 2 + hd / 2 issues of 64 cycles per wave and block); at one wave per SIMD with three barriers
//       per block the measured rate is about a quarter of it: latency between the phases of a block.
//     bf16: q 32 (24) + o 64 (48) + x 16 + prefetch 64 (48) registers; LDS 2 x 32 x (2 hd + 16) B + 16 KB = 50,176 B
//       (41,984 B): hd = 192 runs two workgroups per CU (2 waves per SIMD, 230 registers); hd = 256 is held to 1 wave per
//       SIMD by the register file -- bounded to 256 registers the compiler spilled 64 B per lane, and scratch is not accepted
//       (256 VGPRs + 94 AGPRs, no scratch, as built).  Bound: the staging (fp32 -> bf16 while stored) and the barriers, not
//       the MFMA pipe.
//   There is no byte-mask twin at these widths (ft_attn_fwd stops at 128), hence no bit-equality to it: the tests bound the
//   error against float64.
#include "ft_attn_tile.h"

namespace {

using namespace ft_attn_tile;

__device__ __forceinline__ int clamp_len(const int64_t* lens, int b, int T) {
  const int64_t v = lens[b];
  return v < 0 ? 0 : (v > T ? T : (int)v);
}

// One 64-key block of the online softmax on the transposed score tiles x[kt][e] = key 32 kt + crow(e, hf), query l31:
// scaled to the log2 domain, masked by pm (bit k = key k of the block is masked), m / l updated; x becomes the
// probabilities exp2(x - m_new); -> the factor the accumulated output has to be rescaled by.  The expressions are those
// of ft_attn_fwd_kernel at p_drop = 0, in its order.
__device__ __forceinline__ float online_softmax(f32x16 (&x)[2], unsigned long long pm, float c, int hf, float& m, float& l) {
  float mloc = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kk = 32 * kt + crow(e, hf);
      const float v = ((pm >> kk) & 1ull) ? -INFINITY : x[kt][e] * c;
      x[kt][e] = v;
      mloc = fmaxf(mloc, v);
    }
  mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
  const float mnew = fmaxf(m, mloc);
  const float msafe = mnew == -INFINITY ? 0.f : mnew;
  const float alpha = exp2f(m - msafe);       // m = -inf: 0
  m = mnew;
  float lsum = 0.f;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float p = __builtin_amdgcn_exp2f(x[kt][e] - msafe);
      lsum += p;
      x[kt][e] = p;
    }
  l = l * alpha + lsum;
  return alpha;
}

// rows of att: lane (query l31, half hf) stores columns 32 dt + 8 g + 4 hf .. + 3 of its query's head
template <int DT>
__device__ __forceinline__ void store_rows(float* orow, const f32x16 (&o)[DT], float inv, int hf) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 v = make_float4(o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv, o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
      *reinterpret_cast<float4*>(orow + 32 * dt + 8 * g + 4 * hf) = v;
    }
}

template <int DT>
__device__ __forceinline__ void store_zero_rows(float* orow, int hf) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<float4*>(orow + 32 * dt + 8 * g + 4 * hf) = z;
}

// ---------------------------------------------------------------------------------------------------
// bf16 = 1
// ---------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256, HD > 64 ? 1 : 2) void ft_attn_lens_bf16_kernel(const float* __restrict__ qkv,
                                                                                   const int64_t* __restrict__ lens,
                                                                                   float* __restrict__ att, int T, int nh,
                                                                                   int dmodel, float scale) {
  typedef Tile<HD> TL;
  constexpr int DT = HD / 32, KS = HD / 16;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TL::BYTES];
  unsigned char* Kt = smem;
  unsigned char* Vt = smem + TL::BYTES;
  const int inst = blockIdx.y, b = inst / nh, h = inst - b * nh;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
  const int myq = blockIdx.x * 128 + wave * 32 + l31;
  const int L = clamp_len(lens, b, T);
  float* orow = att + ((long)b * T + myq) * dmodel + h * HD;
  if ((int)blockIdx.x * 128 >= L) {            // every query of this workgroup lies in the padding: zeros, no key loop
    if (myq < T) store_zero_rows<DT>(orow, hf);
    return;
  }
  const long ld = 3L * dmodel;
  const float* qbase = qkv + (long)b * T * ld + h * HD;
  const float* kbase = qbase + dmodel;
  const float* vbase = qbase + 2 * dmodel;
  const float c = scale * LOG2E;

  bf16x8 qf[KS];                               // B operand of X = K Q^T: lane (query l31, hf): d = 16 ks + 8 hf + j
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = load_frag(qbase + (long)myq * ld + 16 * ks + 8 * hf, myq < L);

  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = -INFINITY, l = 0.f;

  const int nkb = (L + KB - 1) / KB;           // the item's own key blocks
  float4 rk[TL::F4], rv[TL::F4];
  TL::load(rk, kbase, ld, 0, L, tid);          // (rows beyond L, not T, read as zeros)
  TL::load(rv, vbase, ld, 0, L, tid);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();                           // the previous block's fragment reads are done
    TL::store(Kt, rk, tid);
    TL::store(Vt, rv, tid);
    __syncthreads();
    if (kb + 1 < nkb) {                        // next block's loads fly during this block's MFMAs
      TL::load(rk, kbase, ld, (kb + 1) * KB, L, tid);
      TL::load(rv, vbase, ld, (kb + 1) * KB, L, tid);
    }
    const unsigned long long pm = pad_mask64(nullptr, kb * KB, L, lane);
    f32x16 x[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) x[kt][e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::row_frag(Kt, 32 * kt + l31, ks, hf), qf[ks], x[kt], 0, 0, 0);
    }
    const float alpha = online_softmax(x, pm, c, hf, m, l);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
    // O^T[d][query] += V^T[d][key] P[key][query]
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pf = acc_frag(x[kt], s);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::tr_frag(Vt, 32 * kt + 16 * s, 32 * dt, lane), pf, o[dt], 0, 0, 0);
      }
  }
  l += __shfl_xor(l, 32, 64);
  if (myq < L)
    store_rows<DT>(orow, o, 1.0f / l, hf);
  else if (myq < T)
    store_zero_rows<DT>(orow, hf);
}

// ---------------------------------------------------------------------------------------------------
// bf16 = 0: fp32-exact products (v_mfma_f32_32x32x2_f32)
// ---------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256, HD > 64 ? 1 : 2) void ft_attn_lens_f32_kernel(const float* __restrict__ qkv,
                                                                                  const int64_t* __restrict__ lens,
                                                                                  float* __restrict__ att, int T, int nh,
                                                                                  int dmodel, float scale) {
  typedef Tile<HD> TL;                         // (its global -> register loader only; the LDS image here is fp32)
  constexpr int DT = HD / 32, NJ = HD / 8;
  constexpr int KRS = HD + 4, VRS = HD + 8;    // row strides in floats (file header)
  __shared__ __attribute__((aligned(16))) float Kt[KB * KRS];
  __shared__ __attribute__((aligned(16))) float Vt[KB * VRS];
  const int inst = blockIdx.y, b = inst / nh, h = inst - b * nh;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
  const int myq = blockIdx.x * 128 + wave * 32 + l31;
  const int L = clamp_len(lens, b, T);
  float* orow = att + ((long)b * T + myq) * dmodel + h * HD;
  if ((int)blockIdx.x * 128 >= L) {
    if (myq < T) store_zero_rows<DT>(orow, hf);
    return;
  }
  const long ld = 3L * dmodel;
  const float* qbase = qkv + (long)b * T * ld + h * HD;
  const float* kbase = qbase + dmodel;
  const float* vbase = qbase + 2 * dmodel;
  const float c = scale * LOG2E;

  float4 qf[NJ];                               // B operand of X: lane (query l31, hf): d = 8 j + 4 hf + i
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    qf[j] = myq < L ? *reinterpret_cast<const float4*>(qbase + (long)myq * ld + 8 * j + 4 * hf) : make_float4(0.f, 0.f, 0.f, 0.f);

  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = -INFINITY, l = 0.f;

  auto stage = [&](float* tile, int rs, const float4 (&r)[TL::F4]) {
#pragma unroll
    for (int i = 0; i < TL::F4; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / (HD / 4), c4 = idx - row * (HD / 4);
      *reinterpret_cast<float4*>(tile + row * rs + 4 * c4) = r[i];
    }
  };

  const int nkb = (L + KB - 1) / KB;
  float4 rk[TL::F4], rv[TL::F4];
  TL::load(rk, kbase, ld, 0, L, tid);
  TL::load(rv, vbase, ld, 0, L, tid);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    stage(Kt, KRS, rk);
    stage(Vt, VRS, rv);
    __syncthreads();
    if (kb + 1 < nkb) {
      TL::load(rk, kbase, ld, (kb + 1) * KB, L, tid);
      TL::load(rv, vbase, ld, (kb + 1) * KB, L, tid);
    }
    const unsigned long long pm = pad_mask64(nullptr, kb * KB, L, lane);
    // X[key][query] = K Q^T: step (j, i) multiplies feature 8 j + 4 hf + i of key l31 (A) and of query l31 (B)
    f32x16 x[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) x[kt][e] = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const float4 a = *reinterpret_cast<const float4*>(Kt + (32 * kt + l31) * KRS + 8 * j + 4 * hf);
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qf[j].x, x[kt], 0, 0, 0);
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qf[j].y, x[kt], 0, 0, 0);
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qf[j].z, x[kt], 0, 0, 0);
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qf[j].w, x[kt], 0, 0, 0);
      }
    const float alpha = online_softmax(x, pm, c, hf, m, l);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
    // O^T[d][query] += V^T[d][key] P[key][query]: step e covers the keys crow(e, 0), crow(e, 1) of the 32-key tile
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float* vrow = Vt + (32 * kt + crow(e, hf)) * VRS + l31;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * dt], x[kt][e], o[dt], 0, 0, 0);
      }
  }
  l += __shfl_xor(l, 32, 64);
  if (myq < L)
    store_rows<DT>(orow, o, 1.0f / l, hf);
  else if (myq < T)
    store_zero_rows<DT>(orow, hf);
}

// ---------------------------------------------------------------------------------------------------
// head widths 192 / 256: 32-key blocks, a pair of waves per 32 queries, the head width split between them (file header)
// ---------------------------------------------------------------------------------------------------
constexpr int WKB = 32;                        // keys per block
constexpr int WQ = 64;                         // queries per workgroup

// online_softmax for ONE 32-key score tile x[e] = key crow(e, hf), query l31; pm: bit k = key k of the block is masked
__device__ __forceinline__ float online_softmax32(f32x16& x, unsigned pm, float c, int hf, float& m, float& l) {
  float mloc = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float v = ((pm >> crow(e, hf)) & 1u) ? -INFINITY : x[e] * c;
    x[e] = v;
    mloc = fmaxf(mloc, v);
  }
  mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
  const float mnew = fmaxf(m, mloc);
  const float msafe = mnew == -INFINITY ? 0.f : mnew;
  const float alpha = exp2f(m - msafe);       // m = -inf: 0
  m = mnew;
  float lsum = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float p = __builtin_amdgcn_exp2f(x[e] - msafe);
    lsum += p;
    x[e] = p;
  }
  l = l * alpha + lsum;
  return alpha;
}

// x += the partial score tile of the other wave of the pair; xs: one [16][64] float tile per wave.  Holds a barrier: every
// wave of the workgroup calls it.  The caller's next barrier orders these reads before the next block's writes.
__device__ __forceinline__ void add_pair_partial(float* xs, f32x16& x, int wave, int lane) {
  float* mine = xs + wave * 1024 + lane;
#pragma unroll
  for (int e = 0; e < 16; ++e) mine[64 * e] = x[e];
  __syncthreads();
  const float* other = xs + (wave ^ 1) * 1024 + lane;
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] += other[64 * e];
}

template <int HD>
__global__ __launch_bounds__(256, HD > 192 ? 1 : 2) void ft_attn_lens_wide_bf16_kernel(const float* __restrict__ qkv,
                                                                         const int64_t* __restrict__ lens,
                                                                         float* __restrict__ att, int T, int nh, int dmodel,
                                                                         float scale) {
  typedef Tile<HD, WKB> TL;
  constexpr int HH = HD / 2, DT = HH / 32, KS = HH / 16;     // the wave's share of the head width
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TL::BYTES];
  __shared__ __attribute__((aligned(16))) float xs[4 * 1024];
  unsigned char* Kt = smem;
  unsigned char* Vt = smem + TL::BYTES;
  const int inst = blockIdx.y, b = inst / nh, h = inst - b * nh;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
  const int pair = wave >> 1, half = wave & 1;
  const int myq = blockIdx.x * WQ + pair * 32 + l31;
  const int L = clamp_len(lens, b, T);
  float* orow = att + ((long)b * T + myq) * dmodel + h * HD + half * HH;
  if ((int)blockIdx.x * WQ >= L) {             // every query of this workgroup lies in the padding: zeros, no key loop
    if (myq < T) store_zero_rows<DT>(orow, hf);
    return;
  }
  const long ld = 3L * dmodel;
  const float* qbase = qkv + (long)b * T * ld + h * HD;
  const float* kbase = qbase + dmodel;
  const float* vbase = qbase + 2 * dmodel;
  const float c = scale * LOG2E;

  bf16x8 qf[KS];                               // lane (query l31, hf): d = half HH + 16 ks + 8 hf + j
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = load_frag(qbase + (long)myq * ld + half * HH + 16 * ks + 8 * hf, myq < L);

  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = -INFINITY, l = 0.f;

  const int nkb = (L + WKB - 1) / WKB;         // the item's own key blocks
  float4 rk[TL::F4], rv[TL::F4];
  TL::load(rk, kbase, ld, 0, L, tid);          // (rows beyond L, not T, read as zeros)
  TL::load(rv, vbase, ld, 0, L, tid);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();                           // the previous block's fragment and exchange reads are done
    TL::store(Kt, rk, tid);
    TL::store(Vt, rv, tid);
    __syncthreads();
    if (kb + 1 < nkb) {
      TL::load(rk, kbase, ld, (kb + 1) * WKB, L, tid);
      TL::load(rv, vbase, ld, (kb + 1) * WKB, L, tid);
    }
    const unsigned pm = (unsigned)pad_mask64(nullptr, kb * WKB, L, lane);      // (bits 0..31: this block's keys)
    f32x16 x;
#pragma unroll
    for (int e = 0; e < 16; ++e) x[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::row_frag(Kt, l31, half * KS + ks, hf), qf[ks], x, 0, 0, 0);
    add_pair_partial(xs, x, wave, lane);
    const float alpha = online_softmax32(x, pm, c, hf, m, l);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
    // O^T[d][query] += V^T[d][key] P[key][query] over the wave's columns d
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 pf = acc_frag(x, s);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::tr_frag(Vt, 16 * s, half * HH + 32 * dt, lane), pf, o[dt], 0, 0, 0);
    }
  }
  l += __shfl_xor(l, 32, 64);
  if (myq < L)
    store_rows<DT>(orow, o, 1.0f / l, hf);
  else if (myq < T)
    store_zero_rows<DT>(orow, hf);
}

template <int HD>
__global__ __launch_bounds__(256, 1) void ft_attn_lens_wide_f32_kernel(const float* __restrict__ qkv,
                                                                        const int64_t* __restrict__ lens,
                                                                        float* __restrict__ att, int T, int nh, int dmodel,
                                                                        float scale) {
  typedef Tile<HD, WKB> TL;                    // (its global -> register loader only; the LDS image here is fp32)
  constexpr int HH = HD / 2, DT = HH / 32, NJ = HH / 8;
  constexpr int KRS = HD + 4, VRS = HD + 8;    // row strides in floats, as in the narrow kernel
  __shared__ __attribute__((aligned(16))) float Kt[WKB * KRS];
  __shared__ __attribute__((aligned(16))) float Vt[WKB * VRS];
  __shared__ __attribute__((aligned(16))) float xs[4 * 1024];
  const int inst = blockIdx.y, b = inst / nh, h = inst - b * nh;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
  const int pair = wave >> 1, half = wave & 1;
  const int myq = blockIdx.x * WQ + pair * 32 + l31;
  const int L = clamp_len(lens, b, T);
  float* orow = att + ((long)b * T + myq) * dmodel + h * HD + half * HH;
  if ((int)blockIdx.x * WQ >= L) {
    if (myq < T) store_zero_rows<DT>(orow, hf);
    return;
  }
  const long ld = 3L * dmodel;
  const float* qbase = qkv + (long)b * T * ld + h * HD;
  const float* kbase = qbase + dmodel;
  const float* vbase = qbase + 2 * dmodel;
  const float c = scale * LOG2E;

  float4 qf[NJ];                               // lane (query l31, hf): d = half HH + 8 j + 4 hf + i
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    qf[j] = myq < L ? *reinterpret_cast<const float4*>(qbase + (long)myq * ld + half * HH + 8 * j + 4 * hf)
                    : make_float4(0.f, 0.f, 0.f, 0.f);

  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = -INFINITY, l = 0.f;

  auto stage = [&](float* tile, int rs, const float4 (&r)[TL::F4]) {
#pragma unroll
    for (int i = 0; i < TL::F4; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / (HD / 4), c4 = idx - row * (HD / 4);
      *reinterpret_cast<float4*>(tile + row * rs + 4 * c4) = r[i];
    }
  };

  const int nkb = (L + WKB - 1) / WKB;
  float4 rk[TL::F4], rv[TL::F4];
  TL::load(rk, kbase, ld, 0, L, tid);
  TL::load(rv, vbase, ld, 0, L, tid);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    stage(Kt, KRS, rk);
    stage(Vt, VRS, rv);
    __syncthreads();
    if (kb + 1 < nkb) {
      TL::load(rk, kbase, ld, (kb + 1) * WKB, L, tid);
      TL::load(rv, vbase, ld, (kb + 1) * WKB, L, tid);
    }
    const unsigned pm = (unsigned)pad_mask64(nullptr, kb * WKB, L, lane);
    // partial X[key][query] over the wave's features: step (j, i) multiplies feature half HH + 8 j + 4 hf + i
    f32x16 x;
#pragma unroll
    for (int e = 0; e < 16; ++e) x[e] = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const float4 a = *reinterpret_cast<const float4*>(Kt + l31 * KRS + half * HH + 8 * j + 4 * hf);
      x = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qf[j].x, x, 0, 0, 0);
      x = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qf[j].y, x, 0, 0, 0);
      x = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qf[j].z, x, 0, 0, 0);
      x = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qf[j].w, x, 0, 0, 0);
    }
    add_pair_partial(xs, x, wave, lane);
    const float alpha = online_softmax32(x, pm, c, hf, m, l);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
    // O^T[d][query] += V^T[d][key] P[key][query]: step e covers the keys crow(e, 0), crow(e, 1)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float* vrow = Vt + crow(e, hf) * VRS + half * HH + l31;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * dt], x[e], o[dt], 0, 0, 0);
    }
  }
  l += __shfl_xor(l, 32, 64);
  if (myq < L)
    store_rows<DT>(orow, o, 1.0f / l, hf);
  else if (myq < T)
    store_zero_rows<DT>(orow, hf);
}

template <int HD>
void launch_wide(const float* qkv, const int64_t* lens, float* att, int B, int T, int nheads, float scale, int bf16,
                 hipStream_t s) {
  const dim3 grid(ft_cdiv(T, WQ), B * nheads);
  if (bf16)
    hipLaunchKernelGGL(ft_attn_lens_wide_bf16_kernel<HD>, grid, dim3(256), 0, s, qkv, lens, att, T, nheads, nheads * HD, scale);
  else
    hipLaunchKernelGGL(ft_attn_lens_wide_f32_kernel<HD>, grid, dim3(256), 0, s, qkv, lens, att, T, nheads, nheads * HD, scale);
}

}  // namespace

extern "C" {

int ft_attn_fwd_lens(const float* qkv, const int64_t* lens, float* att, int B, int T, int nheads, int hd, float scale,
                     int bf16, void* stream) {
  FT_REQUIRE(hd == 64 || hd == 128 || hd == 192 || hd == 256, "attn_fwd_lens: head_dim %d (64, 128, 192 or 256)", hd);
  FT_REQUIRE(B >= 0 && T >= 0 && nheads >= 1 && lens != nullptr, "attn_fwd_lens: bad arguments");
  FT_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)att % 16) == 0, "attn_fwd_lens: buffers must be 16-byte aligned");
  if (B == 0 || T == 0) return FT_OK;
  const dim3 grid(ft_cdiv(T, 128), B * nheads);
  FT_REQUIRE(grid.y <= 65535, "attn_fwd_lens: too many (batch, head) instances");
  const int dmodel = nheads * hd;
  hipStream_t s = (hipStream_t)stream;
  if (hd > 128) {                              // the wide-head layout (file header)
    if (hd == 256)
      launch_wide<256>(qkv, lens, att, B, T, nheads, scale, bf16, s);
    else
      launch_wide<192>(qkv, lens, att, B, T, nheads, scale, bf16, s);
  } else if (bf16) {
    if (hd == 128)
      hipLaunchKernelGGL(ft_attn_lens_bf16_kernel<128>, grid, dim3(256), 0, s, qkv, lens, att, T, nheads, dmodel, scale);
    else
      hipLaunchKernelGGL(ft_attn_lens_bf16_kernel<64>, grid, dim3(256), 0, s, qkv, lens, att, T, nheads, dmodel, scale);
  } else {
    if (hd == 128)
      hipLaunchKernelGGL(ft_attn_lens_f32_kernel<128>, grid, dim3(256), 0, s, qkv, lens, att, T, nheads, dmodel, scale);
    else
      hipLaunchKernelGGL(ft_attn_lens_f32_kernel<64>, grid, dim3(256), 0, s, qkv, lens, att, T, nheads, dmodel, scale);
  }
  return ft_check_launch("attn_fwd_lens");
}

}  // extern "C"
