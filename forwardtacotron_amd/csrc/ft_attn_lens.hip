// Length-aware fused self-attention for inference on a RAGGED batch (generate_batch of the FastPitch models): att =
// softmax(scale Q K^T over the item's own keys) V between the in- and the out-projection, with the item lengths read on the
// device.
//   item b, L = min(max(lens[b], 0), T):  rows t < L of att hold the attention over keys < L, rows t >= L hold exactly 0.
// What lies past an item's length costs nothing and cannot leak: a workgroup whose queries are all at t >= L stores its
// zeros and leaves, every other workgroup's key loop ends at the item's last key block, and every load of a qkv row is
// guarded on L (rows at t >= L arrive as zeros in registers -- a NaN in the padding never meets a multiplication).
// No dropout, no log-sum-exp, no byte mask: the training kernels are in ft_attn.hip.
//
// ONE kernel, ft_attn_lens_kernel<Ops, HD, SPLIT, waves per SIMD>, in the orientation of ft_attn_fwd_kernel (score tile
// transposed, X = K Q^T [32 keys x 32 queries], query on the lane, online softmax in-lane plus one exchange between the
// lane halves, O^T += V^T P); the online softmax is that kernel's own code, online_softmax<KT> of ft_attn_tile.h, called
// here without its dropout.  Per key block: stage K and V (registers -> LDS), barrier, next block's global loads in flight,
// X, [SPLIT = 2: exchange, barrier,] softmax, rescale of O, O^T += V^T P.  Two independent axes:
//
// SPLIT, how a workgroup of 4 waves divides the work.
//   SPLIT = 1 (head widths 64, 128): 128 queries, keys in blocks of 64 (two score tiles); a wave owns 32 queries and the
//     whole head width.
//   SPLIT = 2 (head widths 192, 256: the multispeaker models, 384 / 2 heads in the predictors, 512 / 2 heads in the trunk):
//     the layout above does not stretch -- fp32 q and o alone would be 256 registers per lane at hd = 256, the 64-key K + V
//     tiles 134 KB.  64 queries, keys in blocks of 32 (one score tile), TWO PAIRS of waves; the two waves of a pair share the
//     pair's 32 queries and split the HEAD WIDTH: wave `half` holds features [half hd/2, (half + 1) hd/2) of its queries,
//     forms the PARTIAL score tile over those features, and owns those columns of O.  The two partial tiles are summed
//     through LDS (one 4 KB tile per wave, 16 KB per workgroup; x = own + other, which is the same fp32 sum in both waves
//     because the addition commutes), so both waves of a pair carry identical m, l and probabilities, and no product is
//     formed twice.  The exchange holds a third barrier per block.
//
// Ops, the precision: the form of the query fragment, the LDS image of the K and V tiles and the two MFMA products.
//   Bf16Ops (bf16 = 1): the arithmetic of ft_attn_fwd_kernel, instruction for instruction (operands rounded to bf16 while
//     staged, v_mfma_f32_32x32x16_bf16, same key permutation and block order, the Tile<> image and fragment reads of
//     ft_attn_tile.h).  At SPLIT = 1 valid rows are bit-equal to ft_attn_fwd with the byte mask t >= L at p_drop = 0 -- a
//     fully masked key block there leaves m, l and o unchanged, a masked key inside a block contributes p = 0 either way.
//     There is no byte-mask twin at SPLIT = 2 (ft_attn_fwd stops at 128), hence no bit-equality to it: the tests bound the
//     error against float64.
//   F32Ops (bf16 = 0): fp32-exact products on the fp32-input MFMA v_mfma_f32_32x32x2_f32 (same C/D layout, so the same
//     softmax).  K and V tiles are fp32 row-major in LDS.  X: lane (key or query l31, half hf) covers the features
//     8 j + 4 hf + i of its row (one 16-byte read per four MFMA steps; A from the K tile, B = the query's registers).
//     O^T += V^T P: register e of the probability tile holds key crow(e, hf) for query l31 -- as it stands the B operand of
//     one 32x32x2 step over the keys crow(e, 0), crow(e, 1); the A operand V[crow(e, hf)][32 dt + l31] is a plain read of
//     consecutive floats of one V row per lane half: no shuffle, no transposing read.
//     Row strides: K rows HD + 4 floats (16 lanes x 16 bytes of a b128 read phase tile the 64 banks), V rows HD + 8 floats
//     (the two lane halves read rows 4 apart: 4 * (HD + 8) = 32 mod 64 banks, so they do not meet).
//
// Budget per lane / workgroup, as the compiler reports it in DESIGN.md section 7 (no instantiation uses scratch):
//   F32Ops, SPLIT = 1: hd = 128: 33.0 + 34.0 KB of tiles, one workgroup per CU, 1 wave per SIMD (the 512-register budget
//     holds q (64) + o (64) + x (32) + the 64 prefetch registers); hd = 64: 17.0 + 18.0 KB, 2 waves per SIMD.
//     Bound: the MFMA pipe -- 32x32x2 issues every 64 cycles, 384 of them per wave and 64-key block at hd = 128 (1/16 of
//     the bf16 rate); the T = 840 frame-side layer is 23 GFLOP of the chip's ~157 TF fp32 MFMA peak.
//   F32Ops, SPLIT = 2 (hd = 256; 192 in brackets): q 64 (48) + o 64 (48) + x 16 + K and V prefetch 64 (48) registers; LDS
//     32 x (hd + 4) + 32 x (hd + 8) floats + 16 KB exchange = 83,456 B (67,072 B): one workgroup per CU, 1 wave per SIMD --
//     the LDS, not the register file, sets the occupancy.  Ceiling: the 32x32x2 MFMA pipe as at SPLIT = 1 (hd / 2 + hd / 2
//     issues of 64 cycles per wave and block); at one wave per SIMD with three barriers per block the measured rate is about
//     a quarter of it: latency between the phases of a block.
//   Bf16Ops, SPLIT = 1: 2 x 64 x (2 hd + 16) B = 34,816 B (hd = 128, 1 wave per SIMD) and 18,432 B (hd = 64, 2 waves).
//   Bf16Ops, SPLIT = 2: q 32 (24) + o 64 (48) + x 16 + prefetch 64 (48) registers; LDS 2 x 32 x (2 hd + 16) B + 16 KB =
//     50,176 B (41,984 B): hd = 192 runs two workgroups per CU (2 waves per SIMD); hd = 256 is held to 1 wave per SIMD by
//     the register file -- bounded to 256 registers the compiler spilled 64 B per lane, and scratch is not accepted.
//     Bound: the staging (fp32 -> bf16 while stored) and the barriers, not the MFMA pipe.
#include "ft_attn_tile.h"

namespace {

using namespace ft_attn_tile;

__device__ __forceinline__ int clamp_len(const int64_t* lens, int b, int T) {
  const int64_t v = lens[b];
  return v < 0 ? 0 : (v > T ? T : (int)v);
}

// ---------------------------------------------------------------------------------------------------
// The precisions.  Ops<HD, ROWS, HH>: tiles of ROWS keys x HD features; the calling wave covers the HH features from
// half * HH on (HH = HD, half = 0 unless the head width is split).  KT score tiles per key block, DT output tiles per wave.
// ---------------------------------------------------------------------------------------------------
template <int HD, int ROWS, int HH>
struct Bf16Ops {
  typedef Tile<HD, ROWS> TL;
  static constexpr int KT = ROWS / 32, DT = HH / 32, KS = HH / 16;
  static constexpr int LDS_BYTES = 2 * TL::BYTES;
  struct Q { bf16x8 f[KS]; };                  // B operand of X = K Q^T: lane (query l31, hf): d = half HH + 16 ks + 8 hf + j

  // qrow: the wave's first feature of the lane's query row; zeros if !ok
  __device__ static void load_q(Q& q, const float* qrow, bool ok, int hf) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) q.f[ks] = load_frag(qrow + 16 * ks + 8 * hf, ok);
  }
  __device__ static void stage(unsigned char* smem, const float4 (&rk)[TL::F4], const float4 (&rv)[TL::F4], int tid) {
    TL::store(smem, rk, tid);
    TL::store(smem + TL::BYTES, rv, tid);
  }
  __device__ static void scores(const unsigned char* smem, const Q& q, f32x16 (&x)[KT], int half, int lane) {
    const int l31 = lane & 31, hf = lane >> 5;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) x[kt][e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::row_frag(smem, 32 * kt + l31, half * KS + ks, hf), q.f[ks], x[kt],
                                                        0, 0, 0);
    }
  }
  // O^T[d][query] += V^T[d][key] P[key][query] over the wave's columns d
  __device__ static void accumulate(const unsigned char* smem, const f32x16 (&x)[KT], f32x16 (&o)[DT], int half, int lane) {
    const unsigned char* Vt = smem + TL::BYTES;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pf = acc_frag(x[kt], s);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::tr_frag(Vt, 32 * kt + 16 * s, half * HH + 32 * dt, lane), pf, o[dt],
                                                          0, 0, 0);
      }
  }
};

template <int HD, int ROWS, int HH>
struct F32Ops {
  typedef Tile<HD, ROWS> TL;                   // (its global -> register loader only; the LDS image here is fp32)
  static constexpr int KT = ROWS / 32, DT = HH / 32, NJ = HH / 8;
  static constexpr int KRS = HD + 4, VRS = HD + 8;        // row strides in floats (file header)
  static constexpr int LDS_BYTES = ROWS * (KRS + VRS) * 4;
  struct Q { float4 f[NJ]; };                  // B operand of X: lane (query l31, hf): d = half HH + 8 j + 4 hf + i

  __device__ static void load_q(Q& q, const float* qrow, bool ok, int hf) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      q.f[j] = ok ? *reinterpret_cast<const float4*>(qrow + 8 * j + 4 * hf) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __device__ static void stage_rows(float* tile, int rs, const float4 (&r)[TL::F4], int tid) {
#pragma unroll
    for (int i = 0; i < TL::F4; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / (HD / 4), c4 = idx - row * (HD / 4);
      *reinterpret_cast<float4*>(tile + row * rs + 4 * c4) = r[i];
    }
  }
  __device__ static void stage(unsigned char* smem, const float4 (&rk)[TL::F4], const float4 (&rv)[TL::F4], int tid) {
    float* Kt = reinterpret_cast<float*>(smem);
    stage_rows(Kt, KRS, rk, tid);
    stage_rows(Kt + ROWS * KRS, VRS, rv, tid);
  }
  // X[key][query] = K Q^T over the wave's features: step (j, i) multiplies feature half HH + 8 j + 4 hf + i of key l31 (A)
  // and of query l31 (B)
  __device__ static void scores(const unsigned char* smem, const Q& q, f32x16 (&x)[KT], int half, int lane) {
    const int l31 = lane & 31, hf = lane >> 5;
    const float* Kt = reinterpret_cast<const float*>(smem);
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) x[kt][e] = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const float4 a = *reinterpret_cast<const float4*>(Kt + (32 * kt + l31) * KRS + half * HH + 8 * j + 4 * hf);
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, q.f[j].x, x[kt], 0, 0, 0);
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, q.f[j].y, x[kt], 0, 0, 0);
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, q.f[j].z, x[kt], 0, 0, 0);
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, q.f[j].w, x[kt], 0, 0, 0);
      }
  }
  // O^T[d][query] += V^T[d][key] P[key][query]: step e covers the keys crow(e, 0), crow(e, 1) of the 32-key tile
  __device__ static void accumulate(const unsigned char* smem, const f32x16 (&x)[KT], f32x16 (&o)[DT], int half, int lane) {
    const int l31 = lane & 31, hf = lane >> 5;
    const float* Vt = reinterpret_cast<const float*>(smem) + ROWS * KRS;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float* vrow = Vt + (32 * kt + crow(e, hf)) * VRS + half * HH + l31;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * dt], x[kt][e], o[dt], 0, 0, 0);
      }
  }
};

// SPLIT = 2: x += the partial score tile of the other wave of the pair; xs: one [16][64] float tile per wave.  Holds a
// barrier: every wave of the workgroup calls it.  The caller's next barrier orders these reads before the next block's writes.
constexpr int XCHG_BYTES = 4 * 1024 * 4;
__device__ __forceinline__ void add_pair_partial(float* xs, f32x16& x, int wave, int lane) {
  float* mine = xs + wave * 1024 + lane;
#pragma unroll
  for (int e = 0; e < 16; ++e) mine[64 * e] = x[e];
  __syncthreads();
  const float* other = xs + (wave ^ 1) * 1024 + lane;
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] += other[64 * e];
}

// ---------------------------------------------------------------------------------------------------
// the kernel (file header): SPLIT waves share 32 queries and split the head width; WPS: waves per SIMD of the launch bounds
// ---------------------------------------------------------------------------------------------------
template <template <int, int, int> class OpsT, int HD, int SPLIT, int WPS>
__global__ __launch_bounds__(256, WPS) void ft_attn_lens_kernel(const float* __restrict__ qkv,
                                                                const int64_t* __restrict__ lens, float* __restrict__ att,
                                                                int T, int nh, int dmodel, float scale) {
  constexpr int ROWS = 64 / SPLIT;             // keys per block
  constexpr int QW = 128 / SPLIT;              // queries per workgroup
  constexpr int HH = HD / SPLIT;               // the wave's share of the head width
  typedef OpsT<HD, ROWS, HH> Ops;
  typedef Tile<HD, ROWS> TL;                   // the global -> register loader of both precisions
  constexpr int KT = Ops::KT, DT = Ops::DT;
  __shared__ __attribute__((aligned(16))) unsigned char smem[Ops::LDS_BYTES + (SPLIT == 2 ? XCHG_BYTES : 0)];
  const int inst = blockIdx.y, b = inst / nh, h = inst - b * nh;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
  const int pair = wave / SPLIT, half = wave % SPLIT;
  const int myq = blockIdx.x * QW + pair * 32 + l31;
  const int L = clamp_len(lens, b, T);
  float* orow = att + ((long)b * T + myq) * dmodel + h * HD + half * HH;
  if ((int)blockIdx.x * QW >= L) {             // every query of this workgroup lies in the padding: zeros, no key loop
    if (myq < T) store_zero_rows<DT>(orow, hf);
    return;
  }
  const long ld = 3L * dmodel;
  const float* qbase = qkv + (long)b * T * ld + h * HD;
  const float* kbase = qbase + dmodel;
  const float* vbase = qbase + 2 * dmodel;
  const float c = scale * LOG2E;

  typename Ops::Q q;
  Ops::load_q(q, qbase + (long)myq * ld + half * HH, myq < L, hf);

  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = -INFINITY, l = 0.f;

  const int nkb = (L + ROWS - 1) / ROWS;       // the item's own key blocks
  float4 rk[TL::F4], rv[TL::F4];
  TL::load(rk, kbase, ld, 0, L, tid);          // (rows beyond L, not T, read as zeros)
  TL::load(rv, vbase, ld, 0, L, tid);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();                           // the previous block's fragment and exchange reads are done
    Ops::stage(smem, rk, rv, tid);
    __syncthreads();
    if (kb + 1 < nkb) {                        // next block's loads fly during this block's MFMAs
      TL::load(rk, kbase, ld, (kb + 1) * ROWS, L, tid);
      TL::load(rv, vbase, ld, (kb + 1) * ROWS, L, tid);
    }
    const unsigned long long pm = pad_mask64(nullptr, kb * ROWS, L, lane);     // (ROWS = 32: bits 0..31 are this block's keys)
    f32x16 x[KT];
    Ops::scores(smem, q, x, half, lane);
    if constexpr (SPLIT == 2) add_pair_partial(reinterpret_cast<float*>(smem + Ops::LDS_BYTES), x[0], wave, lane);
    const float alpha = online_softmax<KT>(x, pm, c, hf, m, l, [](float p, int) { return p; });
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
    Ops::accumulate(smem, x, o, half, lane);
  }
  l += __shfl_xor(l, 32, 64);
  if (myq < L)
    store_rows<DT>(orow, o, hf, 1.0f / l);
  else if (myq < T)
    store_zero_rows<DT>(orow, hf);
}

template <template <int, int, int> class OpsT, int HD, int SPLIT, int WPS>
void launch(const float* qkv, const int64_t* lens, float* att, int B, int T, int nheads, float scale, hipStream_t s) {
  const dim3 grid(ft_cdiv(T, 128 / SPLIT), B * nheads);
  hipLaunchKernelGGL((ft_attn_lens_kernel<OpsT, HD, SPLIT, WPS>), grid, dim3(256), 0, s, qkv, lens, att, T, nheads, nheads * HD,
                     scale);
}

}  // namespace

extern "C" {

int ft_attn_fwd_lens(const float* qkv, const int64_t* lens, float* att, int B, int T, int nheads, int hd, float scale,
                     int bf16, void* stream) {
  FT_REQUIRE(hd == 64 || hd == 128 || hd == 192 || hd == 256, "attn_fwd_lens: head_dim %d (64, 128, 192 or 256)", hd);
  FT_REQUIRE(B >= 0 && T >= 0 && nheads >= 1 && lens != nullptr, "attn_fwd_lens: bad arguments");
  FT_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)att % 16) == 0, "attn_fwd_lens: buffers must be 16-byte aligned");
  if (B == 0 || T == 0) return FT_OK;
  FT_REQUIRE((long)B * nheads <= 65535, "attn_fwd_lens: too many (batch, head) instances");      // grid.y of every split
  // [hd / 64 - 1][bf16]: <precision, head width, SPLIT, waves per SIMD>
  typedef void (*Launch)(const float*, const int64_t*, float*, int, int, int, float, hipStream_t);
  static const Launch table[4][2] = {{launch<F32Ops, 64, 1, 2>, launch<Bf16Ops, 64, 1, 2>},
                                     {launch<F32Ops, 128, 1, 1>, launch<Bf16Ops, 128, 1, 1>},
                                     {launch<F32Ops, 192, 2, 1>, launch<Bf16Ops, 192, 2, 2>},
                                     {launch<F32Ops, 256, 2, 1>, launch<Bf16Ops, 256, 2, 1>}};
  table[hd / 64 - 1][bf16 != 0](qkv, lens, att, B, T, nheads, scale, (hipStream_t)stream);
  return ft_check_launch("attn_fwd_lens");
}

}  // extern "C"
