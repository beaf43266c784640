// Fused self-attention for the FastPitch variant in its bf16 matmul mode (BASELINE configs[2]):
//   nn.MultiheadAttention(d, heads, dropout)(x, x, x, key_padding_mask)   (models/common_layers.py:148-185, :172-174)
// between the in-projection and the out-projection: QK^T -> key-padding-masked softmax -> attention dropout -> PV in ONE
// kernel, flash style -- the [B, heads, T, T] score / probability tensors (181 MB per frame-side layer at the benchmark
// shape) never exist in HBM; the backward recomputes the probabilities from Q, K and the forward's per-row log-sum-exp.
// Operands are the fp32 rows of the interleaved projection buffer qkv [B, T, 3d] (q | k | v, head h at columns h*hd),
// rounded to bf16 while they are staged (what every bf16-mode GEMM of the library does); products on
// v_mfma_f32_32x32x16_bf16, softmax statistics, accumulation and outputs in fp32.
//
// Orientation (cdna_hip_programming.md, "An accumulator tile as the next MFMA's operand"): the score tile is computed
// TRANSPOSED, X = K Q^T [32 keys x 32 queries], so that the query sits on the lane and a lane's 16 registers are keys:
//   * the softmax reductions over the keys are in-lane (plus one exchange between the two lane halves);
//   * P (bf16) is, as it stands, the B operand of O^T += V^T P -- the key order inside a 16-key step is permuted
//     (element j of lane half h = key 16 s + 8 (j >> 2) + 4 h + (j & 3)), so the V^T fragments are gathered in that same
//     order, with the transposing LDS read ds_read_b64_tr_b16 from the row-major V tile.
// Workgroup = 4 waves = 128 queries of one (batch item, head); a wave owns 32 queries; keys in blocks of 64; K / V tiles
// row-major bf16 in LDS (row stride HD*2 + 16 bytes), next block's global loads in flight during the current block's
// MFMAs.  Attention dropout re-derives the counter-based mask of ft_softmax_fwd (index = flat index into [B,h,T,T]).
//
// Backward: ft_attn_bwd_dq_kernel (query on the lane, like the forward: dQ^T += K^T dS) and ft_attn_bwd_dkv_kernel (key
// on the lane: dV^T += dO^T P, dK^T += Q^T dS), each recomputing S and dP = dO V^T; no atomics, nothing summed across
// workgroups: bitwise reproducible.
#include "ft_attn_tile.h"
#include "ft_reduce_plan.h"

namespace {

using namespace ft_attn_tile;


// ---------------------------------------------------------------------------------------------------
// forward.  DROP = (p_drop > 0), decided at the launch: tested per element inside the softmax's callable the switch cost
// 2 to 3 % of the kernel, and hoisted in front of it the hd = 64 instantiation spilled.
// ---------------------------------------------------------------------------------------------------
template <int HD, bool DROP>
__global__ __launch_bounds__(256, HD > 64 ? 1 : 2) void ft_attn_fwd_kernel(const float* __restrict__ qkv,
                                                             const unsigned char* __restrict__ key_pad,
                                                             float* __restrict__ att, float* __restrict__ lse2, int T,
                                                             int nh, int dmodel, float scale, float p_drop, uint64_t seed) {
  typedef Tile<HD> TL;
  constexpr int DT = HD / 32, KS = HD / 16;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TL::BYTES];
  unsigned char* Kt = smem;
  unsigned char* Vt = smem + TL::BYTES;
  const int inst = blockIdx.y, b = inst / nh, h = inst - b * nh;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
  const int myq = blockIdx.x * 128 + wave * 32 + l31;
  const long ld = 3L * dmodel;
  const float* qbase = qkv + (long)b * T * ld + h * HD;
  const float* kbase = qbase + dmodel;
  const float* vbase = qbase + 2 * dmodel;
  const unsigned char* kp = key_pad ? key_pad + (long)b * T : nullptr;
  const float c = scale * LOG2E;
  const float inv_keep = DROP ? 1.0f / (1.0f - p_drop) : 1.0f;

  bf16x8 qf[KS];                               // B operand of X = K Q^T: lane (query l31, hf): d = 16 ks + 8 hf + j
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = load_frag(qbase + (long)myq * ld + 16 * ks + 8 * hf, myq < T);

  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = -INFINITY, l = 0.f;

  const int nkb = (T + KB - 1) / KB;
  float4 rk[TL::F4], rv[TL::F4];
  TL::load(rk, kbase, ld, 0, T, tid);
  TL::load(rv, vbase, ld, 0, T, tid);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();                           // the previous block's fragment reads are done
    TL::store(Kt, rk, tid);
    TL::store(Vt, rv, tid);
    __syncthreads();
    if (kb + 1 < nkb) {                        // next block's loads fly during this block's MFMAs
      TL::load(rk, kbase, ld, (kb + 1) * KB, T, tid);
      TL::load(rv, vbase, ld, (kb + 1) * KB, T, tid);
    }
    const unsigned long long pm = pad_mask64(kp, kb * KB, T, lane);
    // X[key][query] = K Q^T
    f32x16 x[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) x[kt][e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        x[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::row_frag(Kt, 32 * kt + l31, ks, hf), qf[ks], x[kt], 0, 0, 0);
    }
    // online softmax over the keys (ft_attn_tile.h: the code of the inference kernels); what this kernel adds is the
    // attention dropout on the probabilities, behind the row sum
    const float alpha = online_softmax<2>(x, pm, c, hf, m, l, [=](float p, int kk) __attribute__((always_inline)) {
      if constexpr (DROP) {
        const long idx = ((long)inst * T + myq) * T + (kb * KB + kk);
        return ft_dropout_keep(seed, idx, p_drop) ? p * inv_keep : 0.f;
      } else {
        return p;
      }
    });
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
  if (myq < T) {
    store_rows<DT>(att + ((long)b * T + myq) * dmodel + h * HD, o, hf, 1.0f / l);
    if (hf == 0) lse2[(long)inst * T + myq] = m + log2f(l);
  }
}

// delta[inst][q] = sum_d dO[q][d] * O[q][d]   (one thread per (query, head); rows of [B,T,dmodel])
__global__ void ft_attn_delta_kernel(const float* __restrict__ dout, const float* __restrict__ out, float* __restrict__ delta,
                                     int B, int T, int nh, int HD) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * nh * T) return;
  const int q = (int)(i % T);
  const int inst = (int)(i / T), b = inst / nh, h = inst - b * nh;
  const long off = ((long)b * T + q) * (long)(nh * HD) + h * HD;
  float s = 0.f;
  for (int d = 0; d < HD; d += 4) {
    const float4 a = *reinterpret_cast<const float4*>(dout + off + d), o = *reinterpret_cast<const float4*>(out + off + d);
    s += a.x * o.x + a.y * o.y + a.z * o.z + a.w * o.w;
  }
  delta[i] = s;
}

// ---------------------------------------------------------------------------------------------------
// backward, dQ: query on the lane (the forward's orientation).  Per key block: X = K Q^T, Y = V dO^T (= dP^T),
// P = exp2(c X - lse2[query]), dS = P (keep/(1-p) Y - delta[query]), dQ^T[d][query] += K^T[d][key] dS[key][query].
// ---------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256, HD > 64 ? 1 : 2) void ft_attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ datt,
                                                                const unsigned char* __restrict__ key_pad,
                                                                const float* __restrict__ lse2,
                                                                const float* __restrict__ delta, float* __restrict__ dqkv,
                                                                int T, int nh, int dmodel, float scale, float p_drop,
                                                                uint64_t seed) {
  typedef Tile<HD> TL;
  constexpr int DT = HD / 32, KS = HD / 16;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TL::BYTES];
  unsigned char* Kt = smem;
  unsigned char* Vt = smem + TL::BYTES;
  const int inst = blockIdx.y, b = inst / nh, h = inst - b * nh;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
  const int myq = blockIdx.x * 128 + wave * 32 + l31;
  const bool qok = myq < T;
  const long ld = 3L * dmodel;
  const float* qbase = qkv + (long)b * T * ld + h * HD;
  const float* kbase = qbase + dmodel;
  const float* vbase = qbase + 2 * dmodel;
  const unsigned char* kp = key_pad ? key_pad + (long)b * T : nullptr;
  const float c = scale * LOG2E;
  const bool drop = p_drop > 0.f;
  const float inv_keep = drop ? 1.0f / (1.0f - p_drop) : 1.0f;

  bf16x8 qf[KS], gf[KS];                       // Q^T and dO^T fragments of this wave's queries
  const float* grow = datt + ((long)b * T + myq) * dmodel + h * HD;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = load_frag(qbase + (long)myq * ld + 16 * ks + 8 * hf, qok);
    gf[ks] = load_frag(grow + 16 * ks + 8 * hf, qok);
  }
  const float L = qok ? lse2[(long)inst * T + myq] : 0.f;
  const float D = qok ? delta[(long)inst * T + myq] : 0.f;
  f32x16 dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) dq[dt][e] = 0.f;

  const int nkb = (T + KB - 1) / KB;
  float4 rk[TL::F4], rv[TL::F4];
  TL::load(rk, kbase, ld, 0, T, tid);
  TL::load(rv, vbase, ld, 0, T, tid);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    TL::store(Kt, rk, tid);
    TL::store(Vt, rv, tid);
    __syncthreads();
    if (kb + 1 < nkb) {
      TL::load(rk, kbase, ld, (kb + 1) * KB, T, tid);
      TL::load(rv, vbase, ld, (kb + 1) * KB, T, tid);
    }
    const unsigned long long pm = pad_mask64(kp, kb * KB, T, lane);
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      f32x16 x, y;
#pragma unroll
      for (int e = 0; e < 16; ++e) x[e] = 0.f, y[e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::row_frag(Kt, 32 * kt + l31, ks, hf), qf[ks], x, 0, 0, 0);
        y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::row_frag(Vt, 32 * kt + l31, ks, hf), gf[ks], y, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int kk = 32 * kt + crow(e, hf);
        const bool masked = (pm >> kk) & 1ull;
        const float p = masked ? 0.f : __builtin_amdgcn_exp2f(x[e] * c - L);
        float g = y[e];
        if (drop) {
          const long idx = ((long)inst * T + myq) * T + (kb * KB + kk);
          g = ft_dropout_keep(seed, idx, p_drop) ? g * inv_keep : 0.f;
        }
        x[e] = scale * p * (g - D);            // dS[key][query]
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 sf = acc_frag(x, s);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::tr_frag(Kt, 32 * kt + 16 * s, 32 * dt, lane), sf, dq[dt], 0, 0, 0);
      }
    }
  }
  if (qok) store_rows<DT>(dqkv + ((long)b * T + myq) * ld + h * HD, dq, hf);
}

// ---------------------------------------------------------------------------------------------------
// backward, dK and dV: key on the lane.  A wave owns 32 keys (K^T and V^T fragments resident), the workgroup sweeps the
// queries in blocks of 64: X = Q K^T [query][key] with -lse2[query] as the initial accumulator, Y = dO V^T with
// -delta[query]; P = exp2(X), Pd = keep/(1-p) P, dS = scale P (keep/(1-p) Y' ...); dV^T[d][key] += dO^T[d][query] Pd,
// dK^T[d][key] += Q^T[d][query] dS -- both sum over the accumulator tiles' row index: no LDS transpose.
// ---------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256, 1) void ft_attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ datt,
                                                                 const unsigned char* __restrict__ key_pad,
                                                                 const float* __restrict__ lse2,
                                                                 const float* __restrict__ delta, float* __restrict__ dqkv,
                                                                 int T, int nh, int dmodel, float scale, float p_drop,
                                                                 uint64_t seed) {
  typedef Tile<HD> TL;
  constexpr int DT = HD / 32, KS = HD / 16;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TL::BYTES];
  __shared__ float sL[KB], sD[KB];
  unsigned char* Qt = smem;
  unsigned char* Gt = smem + TL::BYTES;        // dO tile
  const int inst = blockIdx.y, b = inst / nh, h = inst - b * nh;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
  const int myk = blockIdx.x * 128 + wave * 32 + l31;
  const bool kok = myk < T;
  const long ld = 3L * dmodel;
  const float* qbase = qkv + (long)b * T * ld + h * HD;
  const float* kbase = qbase + dmodel;
  const float* vbase = qbase + 2 * dmodel;
  const float* gbase = datt + (long)b * T * dmodel + h * HD;
  const bool kmask = !kok || (key_pad && key_pad[(long)b * T + myk] != 0);
  const float c = scale * LOG2E;
  const bool drop = p_drop > 0.f;
  const float inv_keep = drop ? 1.0f / (1.0f - p_drop) : 1.0f;

  bf16x8 kf[KS], vf[KS];                       // B operands: lane (key l31, hf): d = 16 ks + 8 hf + j
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = load_frag(kbase + (long)myk * ld + 16 * ks + 8 * hf, kok);
    vf[ks] = load_frag(vbase + (long)myk * ld + 16 * ks + 8 * hf, kok);
  }
  f32x16 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) dk[dt][e] = 0.f, dv[dt][e] = 0.f;

  const int nqb = (T + KB - 1) / KB;
  float4 rq[TL::F4], rg[TL::F4];
  TL::load(rq, qbase, ld, 0, T, tid);
  TL::load(rg, gbase, dmodel, 0, T, tid);
  for (int qb = 0; qb < nqb; ++qb) {
    __syncthreads();
    TL::store(Qt, rq, tid);
    TL::store(Gt, rg, tid);
    if (tid < KB) {
      const int q = qb * KB + tid;
      sL[tid] = q < T ? lse2[(long)inst * T + q] : INFINITY;      // exp2(x - inf) = 0: rows beyond T contribute nothing
      sD[tid] = q < T ? delta[(long)inst * T + q] : 0.f;
    }
    __syncthreads();
    if (qb + 1 < nqb) {
      TL::load(rq, qbase, ld, (qb + 1) * KB, T, tid);
      TL::load(rg, gbase, dmodel, (qb + 1) * KB, T, tid);
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      f32x16 x, y;
#pragma unroll
      for (int e = 0; e < 16; ++e) x[e] = 0.f, y[e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::row_frag(Qt, 32 * qt + l31, ks, hf), kf[ks], x, 0, 0, 0);
        y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::row_frag(Gt, 32 * qt + l31, ks, hf), vf[ks], y, 0, 0, 0);
      }
      f32x16 pd;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int qq = 32 * qt + crow(e, hf);                       // query (tile row) of this register
        const float p = kmask ? 0.f : __builtin_amdgcn_exp2f(x[e] * c - sL[qq]);
        float keepf = 1.f;
        if (drop) {
          const long idx = ((long)inst * T + (qb * KB + qq)) * T + myk;
          keepf = ft_dropout_keep(seed, idx, p_drop) ? inv_keep : 0.f;
        }
        pd[e] = p * keepf;
        x[e] = scale * p * (y[e] * keepf - sD[qq]);                 // dS[query][key]
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pf = acc_frag(pd, s), sf = acc_frag(x, s);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::tr_frag(Gt, 32 * qt + 16 * s, 32 * dt, lane), pf, dv[dt], 0, 0, 0);
          dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::tr_frag(Qt, 32 * qt + 16 * s, 32 * dt, lane), sf, dk[dt], 0, 0, 0);
        }
      }
    }
  }
  if (kok) {
    float* krow = dqkv + ((long)b * T + myk) * ld + dmodel + h * HD;
    store_rows<DT>(krow, dk, hf);
    store_rows<DT>(krow + dmodel, dv, hf);
  }
}

}  // namespace

extern "C" {

size_t ft_attn_workspace(int B, int T, int nheads) { return reduce_plan::attn_bwd_bytes(B, T, nheads); }

int ft_attn_fwd(const float* qkv, const unsigned char* key_pad, float* att, float* lse2, int B, int T, int nheads, int hd,
                float scale, float p_drop, uint64_t seed, void* stream) {
  FT_REQUIRE(hd == 64 || hd == 128, "attn_fwd: head_dim %d (64 or 128)", hd);
  FT_REQUIRE(B >= 0 && T >= 0 && nheads >= 1 && p_drop >= 0.f && p_drop < 1.f, "attn_fwd: bad arguments");
  FT_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)att % 16) == 0, "attn_fwd: buffers must be 16-byte aligned");
  if (B == 0 || T == 0) return FT_OK;
  const dim3 grid(ft_cdiv(T, 128), B * nheads);
  FT_REQUIRE(grid.y <= 65535, "attn_fwd: too many (batch, head) instances");
  const int dmodel = nheads * hd;
  typedef void (*Kernel)(const float*, const unsigned char*, float*, float*, int, int, int, float, float, uint64_t);
  const Kernel k = hd == 128 ? (p_drop > 0.f ? ft_attn_fwd_kernel<128, true> : ft_attn_fwd_kernel<128, false>)
                             : (p_drop > 0.f ? ft_attn_fwd_kernel<64, true> : ft_attn_fwd_kernel<64, false>);
  hipLaunchKernelGGL(k, grid, dim3(256), 0, (hipStream_t)stream, qkv, key_pad, att, lse2, T, nheads, dmodel, scale, p_drop, seed);
  return ft_check_launch("attn_fwd");
}

int ft_attn_bwd(const float* qkv, const float* att, const float* datt, const unsigned char* key_pad, const float* lse2,
                float* dqkv, int B, int T, int nheads, int hd, float scale, float p_drop, uint64_t seed, void* workspace,
                size_t workspace_bytes, void* stream) {
  FT_REQUIRE(hd == 64 || hd == 128, "attn_bwd: head_dim %d (64 or 128)", hd);
  FT_REQUIRE(B >= 0 && T >= 0 && nheads >= 1 && p_drop >= 0.f && p_drop < 1.f, "attn_bwd: bad arguments");
  FT_REQUIRE(workspace && workspace_bytes >= ft_attn_workspace(B, T, nheads), "attn_bwd: workspace too small");
  if (B == 0 || T == 0) return FT_OK;
  hipStream_t s = (hipStream_t)stream;
  float* delta = (float*)workspace;
  const long n = (long)B * nheads * T;
  hipLaunchKernelGGL(ft_attn_delta_kernel, dim3(ft_cdiv(n, 256)), dim3(256), 0, s, datt, att, delta, B, T, nheads, hd);
  const dim3 grid(ft_cdiv(T, 128), B * nheads);
  FT_REQUIRE(grid.y <= 65535, "attn_bwd: too many (batch, head) instances");
  const int dmodel = nheads * hd;
  if (hd == 128) {
    hipLaunchKernelGGL(ft_attn_bwd_dq_kernel<128>, grid, dim3(256), 0, s, qkv, datt, key_pad, lse2, delta, dqkv, T, nheads,
                       dmodel, scale, p_drop, seed);
    hipLaunchKernelGGL(ft_attn_bwd_dkv_kernel<128>, grid, dim3(256), 0, s, qkv, datt, key_pad, lse2, delta, dqkv, T, nheads,
                       dmodel, scale, p_drop, seed);
  } else {
    hipLaunchKernelGGL(ft_attn_bwd_dq_kernel<64>, grid, dim3(256), 0, s, qkv, datt, key_pad, lse2, delta, dqkv, T, nheads,
                       dmodel, scale, p_drop, seed);
    hipLaunchKernelGGL(ft_attn_bwd_dkv_kernel<64>, grid, dim3(256), 0, s, qkv, datt, key_pad, lse2, delta, dqkv, T, nheads,
                       dmodel, scale, p_drop, seed);
  }
  return ft_check_launch("attn_bwd");
}

}  // extern "C"
