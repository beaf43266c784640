// Internal descriptors for the exact-f32 MFMA GEMM / shifted-row (conv) kernels.
#pragma once
#include "ft_common.h"
#include "ft_gemm_plan.h"      // the descriptors (FtGemmBatch, FtGemmTNTask, FtGemmVariant) and the launch planner

// The highway epilogues (see FtGemmBatch) for an accumulator tile in the 32x32 MFMA layout shared by the row kernels:
// wave (wm, wn) of 2 x 2, lane (half, l31) holds column l31 and rows (e & 3) + 8 * (e >> 2) + 4 * half of each tile.
// lds: >= 2 * 32 * 33 floats of idle LDS (TN == 1 only), safe to overwrite when this is called.  Every thread of the
// workgroup must call it (TN == 1 synchronises).
template <int TM, int TN>
__device__ __forceinline__ void ft_highway_epilogue(const FtGemmBatch& bt, const FtGemmTask& T, float* TC,
                                                    f32x16 (&acc)[TM][TN], float* lds, int m0, int n0, int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int half = lane >> 5, l31 = lane & 31;
  const int C = bt.hw_C, tM = T.M;
  const long ldc = T.ldc;
  const float* hx = bt.hw_x;
  if (bt.hw_mode == 1) {
    float* x12 = bt.hw_x12;
    if constexpr (TN == 2) {
      const int unit = ((n0 + wn * 64) >> 6) * 32 + l31;              // both 32-column tiles of this wave: the same units
      const bool uok = unit < C;
      const float b1 = uok ? bt.hw_b1[unit] : 0.f, b2 = uok ? bt.hw_b2[unit] : 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + wm * 32 * TM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * half;
          if (row >= tM || !uok) continue;
          const float y1 = acc[i][0][e] + b1, y2 = acc[i][1][e] + b2;
          const float g = ft_sigmoid(y2);
          if (x12) {
            x12[(long)row * 2 * C + unit] = y1;
            x12[(long)row * 2 * C + C + unit] = y2;
          }
          TC[(long)row * ldc + unit] = g * fmaxf(y1, 0.f) + (1.f - g) * hx[(long)row * C + unit];
        }
    } else {
      static_assert(TN == 1 || TN == 2, "highway epilogue: 32- or 64-column waves");
      // 64-column tiles: wave wn = 0 holds y1, wave wn = 1 y2 of the same 32 units -> the gate travels through LDS
      const int unit = (n0 >> 6) * 32 + l31;
      const bool uok = unit < C;
      float* gl = lds + wm * (32 * TM) * 33;
      if (wn == 1) {
        const float b2 = uok ? bt.hw_b2[unit] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int rl = 32 * i + (e & 3) + 8 * (e >> 2) + 4 * half;
            const int row = m0 + wm * 32 * TM + rl;
            const float y2 = acc[i][0][e] + b2;
            gl[rl * 33 + l31] = ft_sigmoid(y2);
            if (x12 && row < tM && uok) x12[(long)row * 2 * C + C + unit] = y2;
          }
      }
      __syncthreads();
      if (wn == 0) {
        const float b1 = uok ? bt.hw_b1[unit] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int rl = 32 * i + (e & 3) + 8 * (e >> 2) + 4 * half;
            const int row = m0 + wm * 32 * TM + rl;
            if (row >= tM || !uok) continue;
            const float y1 = acc[i][0][e] + b1;
            const float g = gl[rl * 33 + l31];
            if (x12) x12[(long)row * 2 * C + unit] = y1;
            TC[(long)row * ldc + unit] = g * fmaxf(y1, 0.f) + (1.f - g) * hx[(long)row * C + unit];
          }
      }
    }
    return;
  }
  // mode 2
  const float* x12 = bt.hw_x12;
  float* d12 = bt.hw_d12;
  const bool eacc = T.accumulate != 0;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * 32 * TN + 32 * j + l31;
      if (col >= T.N) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 32 * TM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * half;
        if (row >= tM) continue;
        float* cp = TC + (long)row * ldc + col;
        float dv = acc[i][j][e];
        if (eacc) dv += *cp;
        const float y1 = x12[(long)row * 2 * C + col], y2 = x12[(long)row * 2 * C + C + col];
        const float g = ft_sigmoid(y2);
        d12[(long)row * 2 * C + col] = y1 > 0.f ? dv * g : 0.f;
        d12[(long)row * 2 * C + C + col] = dv * (fmaxf(y1, 0.f) - hx[(long)row * C + col]) * g * (1.f - g);
        *cp = dv * (1.f - g);
      }
    }
}


// Workgroup -> (M-tile, tap, split) of a TN launch.  Plain tasks: blockIdx.x = M-tile, blockIdx.z = (instance*taps +
// tap)*S + split.  Conv-bank mode: member kk only has taps j < kk, so the grid enumerates the LIVE (member, tap, tile)
// triples along x (kk ascending, then tap, then the member's M-tiles) and blockIdx.z = split -- no empty workgroups,
// equal work per workgroup (the round-robin XCD assignment stays balanced), and neighbours share their dy tile.
struct FtTnWho {
  int mtile, zts, s, kk;      // zts = instance*taps + tap ; kk = member (bank mode) or 0
};
__device__ __forceinline__ FtTnWho ft_tn_who(const FtGemmTNTask& T, int S, int BM) {
  FtTnWho w;
  if (T.bankC > 0) {
    const int tpm = T.bankC / BM;                 // M-tiles per member
    const int q = blockIdx.x / tpm, sub = blockIdx.x - q * tpm;
    int kk = 1, first = 0;                        // first = kk(kk-1)/2 = index of (kk, tap 0)
    while (first + kk <= q) {
      first += kk;
      ++kk;
    }
    w.kk = kk;
    w.zts = q - first;
    w.mtile = (kk - 1) * tpm + sub;
    w.s = blockIdx.z;
  } else {
    w.kk = 0;
    w.mtile = blockIdx.x;
    w.zts = blockIdx.z / S;
    w.s = blockIdx.z - w.zts * S;
  }
  return w;
}

extern long g_ft_gemm_variant[FT_GV_COUNT];
static inline void ft_count_variant(int v) { ++g_ft_gemm_variant[v]; }

// the process's FT_GEMM_* / FT_TN_* switches, read from the environment on first use
const gemm_plan::Switches& ft_gemm_switches();
int ft_launch_gemm_rows(FtGemmBatch* batch, int ntasks, bool b_ncontig, hipStream_t stream);
// scratch (floats) a launch of these tasks can use for split-K (0: it would not be split)
size_t ft_rows_ksplit_floats(const FtGemmBatch& batch, int ntasks, hipStream_t stream);
int ft_launch_ksplit_reduce(const float* slab, int S, const FtGemmTask& t, hipStream_t stream);
// One row per kernel instantiation: the planned variant it serves (gemm_plan::plan_rows / plan_tn) and the precision
// (ft_gemm_precision; -1: both).  Each .hip has the table of the kernels it defines; a planned variant without a row
// is an error.
struct FtGemmInstance {
  int variant, precision;
  void (*rows)(FtGemmBatch);
  void (*tn)(FtGemmTNTask, float*, int, int);
};
template <int N>
const FtGemmInstance* ft_gemm_instance(const FtGemmInstance (&table)[N], int variant, int precision) {
  for (const FtGemmInstance& k : table)
    if (k.variant == variant && (k.precision < 0 || k.precision == precision)) return &k;
  ft_set_error("gemm: no kernel for the planned variant %d at precision %d", variant, precision);
  return nullptr;
}
// ft_gemm_b3.hip: the bf16-pipe kernel of a planned variant (FT_GV_ROWS_B3* / FT_GV_TN_B3*)
const FtGemmInstance* ft_gemm_b3_instance(int variant, int precision);
// ft_capi_core.hip: workgroup slots (2 per usable CU) of a stream -- 512 unless it is CU-limited
void ft_note_stream_slots(hipStream_t s, int slots);
int ft_stream_slots(hipStream_t s);
// 0 = fp32-exact (default), 1 = bf16 operands / fp32 accumulate on every NT-form fast launch (ft_set_gemm_precision)
int ft_gemm_precision();
int ft_launch_gemm_tn(const FtGemmTNTask& task, float* workspace, size_t workspace_floats,
                      hipStream_t stream);
size_t ft_gemm_tn_workspace_floats(const FtGemmTNTask& task);
// dst[m*ldm + n] = sum_{s<S} slab[s][m][n]  (fixed order)
int ft_launch_slab_sum(const float* slab, float* dst, int M, int N, int S, long ldm, hipStream_t stream);
