// Training kernels of the Tacotron teacher for gfx950: the backward of the teacher-forced attention recurrence
// (ft_taco_attend, csrc/ft_taco.hip) and the decoder's residual LSTMCells with the reference's zoneout, forward and
// backward (models/tacotron.py:119-122 Decoder.zoneout, :152-166).  DESIGN.md section 7 derives the step.
//
// Every kernel is a plain launch that ends on its own; the host enqueues a fixed chain per step.  No atomics: every
// destination element is owned by one workgroup per launch, and what is summed across workgroups goes through
// per-workgroup slabs that are added once, in ascending order.  The same inputs give the same bits.  All fp32.
//
// ---- zoneout LSTMCell sequence ---------------------------------------------------------------------------------------
//   h_s = m_s h_{s-1} + (1 - m_s) LSTMCell(x_s, (h_{s-1}, c_{s-1})).h     c_s = the cell's c (not zoned)
//   m_s[b,u] = 1 exactly where ft_dropout's mask of (seed, p) is 0 at flat index (s B + b) L + u  (P(m = 1) = p)
// forward, one launch per step: grid (L/4, ceil(B/16)); 16 items x 4 units x (i, f, g, o) = one 16 x 16 tile of
// h_{s-1} W_hh^T on v_mfma_f32_16x16x4_f32, K = L split over the four waves, then the cell and the mix.  Saves the
// activated gates, c and the zoned h.  backward, one launch per step, s = S-1 .. 0: grid (ceil(L/16), ceil(B/16)); the
// tile is dgates_{s+1} W_hh (K = 4L), so dh_s = dout_s + m_{s+1} dh_{s+1} + dgates_{s+1} W_hh is complete when the cell
// backward of step s starts; dh ping-pongs on the parity of s, dc is updated in place by its owner.
//
// ---- attention BPTT --------------------------------------------------------------------------------------------------
// Saved by the forward: hist [S,B,512] = [ctx_s | h_s] and attn [B,S,Tx].  cum_{s-1} comes from a prefix buffer built
// once in the forward's own order of additions; tanh(...) and the GRU gates are recomputed.  Per step, five launches:
//   1. softmax_bwd  (B)             dctx_s = dhist_s[:256] + dctx; q = W h_s + bW + bL; datt = <dctx_s, epq[t]> +
//                                   datt_loc + dcum; de = att (datt - sum att datt); depq[b,t,:] += att[t] dctx_s
//   2. energy_bwd   (chunks of 32 tokens, B)   thread = attention column: a = tanh(q + ep + L loc), g = de v (1 - a^2);
//                                   dep += g; slabs of dq, dv, dL; dloc = g L
//   3. conv_bwd     (chunks, B)     din from dloc over the 31-tap window -> dcum += din[0], datt_loc = din[1]; slab of
//                                   dcw; chunk 0 adds the dq slabs in ascending order -> dq_s
//   4. gru_bwd      (64 unit blocks, ceil(B/16))  the forward's gate product again (16 items x 4 units on the MFMA),
//                                   dh_s = dhist_s[256:] + dh + W^T dq_s, the cell backward -> dP_s = dgx, dgh, z dh_s
//   5. carry        (16, ceil(B/16), 2)   dctx = dgx W_ih[:, :256], dh = dgh W_hh + z dh_s  (s > 0 only)
// After the loop: dW_hh = sum dgh_s^T h_{s-1}, dW_ih[:, :256] = sum dgx_s^T ctx_{s-1}, dW = sum dq_s^T h_s on the TN
// GEMM (ft_linear_bwd_weight), db_hh and dbW = dbL on ft_colsum, and the dv / dL / dcw slabs are added.
#include "ft_common.h"
#include "fwdtaco_hip.h"

namespace {

constexpr int DA = 256;          // decoder / attention dims
constexpr int NG = 3 * DA;       // GRU gate rows
constexpr int NF = 32;           // location filters
constexpr int KW = 31;           // location kernel width (padding 15)
constexpr int KP = KW / 2;
constexpr int UB = 4;            // hidden units per GRU workgroup
constexpr int TC = 32;           // tokens per chunk
constexpr int WIN = TC + KW - 1; // window of a chunk
constexpr int NCW = NF * 2 * KW; // conv weights
constexpr int TXMAX = 1024;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ void mfma4(const float4& a, const float4& b, f32x4& acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

// One 16 x 16 tile sum_k A[i][k] Bm[j][k] by the four waves of a 256-thread workgroup: lane (l15, q) holds row l15 of
// both operands (arow, brow: 16-byte aligned, K % 4 == 0), k = 16c + 4q .. +3; the waves split K in 16-wide chunks and
// the four partial tiles are added in a fixed order.  Returns element (tid >> 4, tid & 15).  Called by all 256 threads.
__device__ __forceinline__ float tile16(const float* arow, const float* brow, int K, float (&red)[4][16][17]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
  const int cpw = ((K + 15) / 16 + 3) / 4 * 16;
  const int k0 = min(K, wave * cpw), k1 = min(K, k0 + cpw);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int kb = k0; kb < k1; kb += 16) {              // wave-uniform trip count
    const int k = kb + 4 * q;
    float4 a = z, b = z;
    if (k < k1) { a = ld4(arow + k); b = ld4(brow + k); }
    mfma4(a, b, acc);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[wave][4 * q + e][l15] = acc[e];
  __syncthreads();
  const int i = tid >> 4, j = tid & 15;
  return (red[0][i][j] + red[1][i][j]) + (red[2][i][j] + red[3][i][j]);
}

__device__ __forceinline__ float block_sum256(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ float wave_all_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- zoneout LSTM ----------------------------------------------------------------------------------------------------
struct ZoneArgs {
  const float* xp;      // [S,B,4L] input projection, b_ih included
  const float* whh;     // [4L,L]
  const float* bhh;     // [4L]
  float* gates;         // [S,B,4L] activated i, f, g, o
  float* c;             // [S,B,L]
  float* h;             // [S,B,L] zoned
  int B, S, L;
  float p;
  uint64_t seed;
};

__global__ __launch_bounds__(256) void ft_lstm_zone_fwd_kernel(ZoneArgs a, int s) {
  __shared__ float red[4][16][17];
  const int B = a.B, L = a.L, b0 = blockIdx.y * 16, u0 = blockIdx.x * UB;
  const int tid = threadIdx.x, l15 = tid & 15;
  float prod = 0.f;                                   // element (item tid >> 4, column tid & 15 = 4 * unit + gate)
  if (s > 0) {
    const float* arow = a.h + ((long)(s - 1) * B + min(b0 + l15, B - 1)) * L;
    const float* brow = a.whh + ((long)(l15 & 3) * L + min(u0 + (l15 >> 2), L - 1)) * L;
    prod = tile16(arow, brow, L, red);
  }
  // thread -> (item, unit, gate): the four gates of a cell sit in four neighbouring lanes
  const int it = tid >> 4, uj = l15 >> 2, gq = l15 & 3, cb = b0 + it, cu = u0 + uj;
  const bool act = cb < B && cu < L;
  float pre = 0.f;
  if (act) pre = (a.xp[((long)s * B + cb) * 4 * L + (long)gq * L + cu] + prod) + a.bhh[gq * L + cu];
  const float gv = gq == 2 ? ft_tanh(pre) : ft_sigmoid(pre);
  const int base = (tid & 63) & ~3;
  const float gi = __shfl(gv, base, 64), gf = __shfl(gv, base + 1, 64), gg = __shfl(gv, base + 2, 64),
              go = __shfl(gv, base + 3, 64);
  if (act) {
    const long e = ((long)s * B + cb) * L + cu;
    a.gates[((long)s * B + cb) * 4 * L + (long)gq * L + cu] = gv;
    if (gq == 0) {
      const float cprev = s > 0 ? a.c[e - (long)B * L] : 0.f;
      const float hprev = s > 0 ? a.h[e - (long)B * L] : 0.f;
      const float c = gf * cprev + gi * gg;
      const float hc = go * ft_tanh(c);
      a.c[e] = c;
      a.h[e] = ft_dropout_keep(a.seed, e, a.p) ? hc : hprev;
    }
  }
}

struct ZoneBwdArgs {
  const float* dout;    // [S,B,L]
  const float* gates;   // [S,B,4L]
  const float* c;       // [S,B,L]
  const float* whhT;    // [L,4L]
  float* dxp;           // [S,B,4L]
  float* dh;            // [2][B,L]
  float* dc;            // [B,L]
  int B, S, L;
  float p;
  uint64_t seed;
};

__global__ __launch_bounds__(256) void ft_lstm_zone_bwd_kernel(ZoneBwdArgs a, int s) {
  __shared__ float red[4][16][17];
  const int B = a.B, L = a.L, S = a.S, b0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  const int tid = threadIdx.x, l15 = tid & 15;
  const bool last = s == S - 1;
  float prod = 0.f;
  if (!last) {
    const float* arow = a.dxp + ((long)(s + 1) * B + min(b0 + l15, B - 1)) * 4 * L;
    const float* brow = a.whhT + (long)min(j0 + l15, L - 1) * 4 * L;
    prod = tile16(arow, brow, 4 * L, red);
  }
  const int cb = b0 + (tid >> 4), cu = j0 + l15;
  if (cb >= B || cu >= L) return;
  const long bl = (long)B * L, o = (long)cb * L + cu, e = (long)s * bl + o;
  float dh = a.dout[e];
  if (!last) {
    const bool zoned1 = !ft_dropout_keep(a.seed, e + bl, a.p);
    dh += prod + (zoned1 ? a.dh[(long)((s + 1) & 1) * bl + o] : 0.f);
  }
  a.dh[(long)(s & 1) * bl + o] = dh;
  const float dhc = ft_dropout_keep(a.seed, e, a.p) ? dh : 0.f;
  const float* g = a.gates + ((long)s * B + cb) * 4 * L + cu;
  const float gi = g[0], gf = g[L], gg = g[2 * L], go = g[3 * L];
  const float tc = ft_tanh(a.c[e]);
  const float cprev = s > 0 ? a.c[e - bl] : 0.f;
  const float dcv = (last ? 0.f : a.dc[o]) + dhc * go * (1.f - tc * tc);
  float* d = a.dxp + ((long)s * B + cb) * 4 * L + cu;
  d[0] = dcv * gg * gi * (1.f - gi);
  d[L] = dcv * cprev * gf * (1.f - gf);
  d[2 * L] = dcv * gi * (1.f - gg * gg);
  d[3 * L] = dhc * tc * go * (1.f - go);
  a.dc[o] = dcv * gf;
}

// ---- attention BPTT ----------------------------------------------------------------------------------------------------
struct AttBwdArgs {
  const float *ep, *epq, *P, *wih; long ld_wih;
  const float *whh, *bhh, *W, *bW, *cw, *L, *bL, *v;
  const float *hist, *attn, *dhist;
  float *dep, *depq, *dP;
  // workspace
  float *wihT, *whhT;               // [256,768] each: W_ih[:, :256]^T, W_hh^T
  float *cumP;                      // [S,B,Tx]  cum_{s-1}
  float *dgh, *dq;                  // [S,B,768], [S,B,256]
  float *q, *de, *dloc, *dcum, *dal, *dctx, *dh, *zdh, *dqp, *dvp, *dLp, *dcwp;
  int B, Tx, S, nch;
};

__global__ void ft_taco_transpose_kernel(const float* __restrict__ src, long lds, int rows, int cols, float* __restrict__ dst) {
  const long n = (long)rows * cols;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i / rows), r = (int)(i % rows);
    dst[i] = src[(long)r * lds + c];                       // dst [cols, rows]
  }
}

// cumP[s] = cum_{s-1}: the forward's own additions, in its order
__global__ void ft_taco_cumprefix_kernel(AttBwdArgs a) {
  const long n = (long)a.B * a.Tx;
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int b = (int)(i / a.Tx), t = (int)(i % a.Tx);
  float cum = 0.f;
  for (int s = 0; s < a.S; ++s) {
    a.cumP[(long)s * n + i] = cum;
    cum += a.attn[((long)b * a.S + s) * a.Tx + t];
  }
}

// 1. context / softmax backward of item b
__global__ __launch_bounds__(256) void ft_taco_softmax_bwd_kernel(AttBwdArgs a, int s) {
  __shared__ __attribute__((aligned(16))) float dctx[DA];
  __shared__ __attribute__((aligned(16))) float hs[DA];
  __shared__ float dat[TXMAX];
  __shared__ float sh[4];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int B = a.B, Tx = a.Tx, S = a.S;
  const long row = (long)s * B + b;
  dctx[tid] = a.dhist[row * 2 * DA + tid] + (s < S - 1 ? a.dctx[(long)b * DA + tid] : 0.f);
  hs[tid] = a.hist[row * 2 * DA + DA + tid];
  __syncthreads();
  const float4 h4 = ld4(&hs[4 * lane]), d4 = ld4(&dctx[4 * lane]);
  for (int i = wave; i < DA; i += 4) {                  // q = W h_s + bW + bL
    const float4 w = ld4(a.W + (long)i * DA + 4 * lane);
    const float v = wave_all_sum((w.x * h4.x + w.y * h4.y) + (w.z * h4.z + w.w * h4.w));
    if (lane == 0) a.q[(long)b * DA + i] = (v + a.bW[i]) + a.bL[i];
  }
  const float* att = a.attn + ((long)b * S + s) * Tx;
  for (int t = wave; t < Tx; t += 4) {
    const long o = ((long)b * Tx + t) * DA + 4 * lane;
    const float4 x = ld4(a.epq + o);
    const float v = wave_all_sum((x.x * d4.x + x.y * d4.y) + (x.z * d4.z + x.w * d4.w));
    const float p = att[t];
    float4 acc = ld4(a.depq + o);
    acc.x = fmaf(p, d4.x, acc.x); acc.y = fmaf(p, d4.y, acc.y); acc.z = fmaf(p, d4.z, acc.z); acc.w = fmaf(p, d4.w, acc.w);
    *reinterpret_cast<float4*>(a.depq + o) = acc;
    if (lane == 0) dat[t] = v + (a.dal[(long)b * Tx + t] + a.dcum[(long)b * Tx + t]);
  }
  __syncthreads();
  float part = 0.f;
  for (int t = tid; t < Tx; t += 256) part = fmaf(att[t], dat[t], part);
  const float dot = block_sum256(part, sh);
  for (int t = tid; t < Tx; t += 256) a.de[(long)b * Tx + t] = att[t] * (dat[t] - dot);
}

// the location window of chunk t0 of item b at step s: [cum_{s-1}, att_{s-1}] at t0 - 15 .. t0 + 46, zero outside
__device__ __forceinline__ void load_window(const AttBwdArgs& a, int s, int b, int t0, float (&locw)[2][WIN]) {
  const int Tx = a.Tx;
  for (int i = threadIdx.x; i < 2 * WIN; i += 256) {
    const int c = i / WIN, o = i - c * WIN, t = t0 - KP + o;
    float v = 0.f;
    if (s > 0 && t >= 0 && t < Tx)
      v = c == 0 ? a.cumP[((long)s * a.B + b) * Tx + t] : a.attn[((long)b * a.S + s - 1) * Tx + t];
    locw[c][o] = v;
  }
}

// 2. energy backward: thread = attention column, the chunk's tokens in turn
__global__ __launch_bounds__(256) void ft_taco_energy_bwd_kernel(AttBwdArgs a, int s) {
  __shared__ float locw[2][WIN];
  __shared__ float cws[NF][2 * KW + 1];
  __shared__ float convs[TC][NF + 1];
  __shared__ float des[TC];
  __shared__ float gs[TC][DA + 1];
  const int ch = blockIdx.x, t0 = ch * TC, b = blockIdx.y, tid = threadIdx.x;
  const int Tx = a.Tx;
  const int nt = min(TC, Tx - t0);
  load_window(a, s, b, t0, locw);
  for (int i = tid; i < NCW; i += 256) cws[i / (2 * KW)][i % (2 * KW)] = a.cw[i];
  if (tid < TC) des[tid] = tid < nt ? a.de[(long)b * Tx + t0 + tid] : 0.f;
  __syncthreads();
  {
    const int f = tid & 31, tb = 4 * (tid >> 5);
    float cv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 2; ++c)
      for (int k = 0; k < KW; ++k) {
        const float w = cws[f][c * KW + k];
#pragma unroll
        for (int i = 0; i < 4; ++i) cv[i] = fmaf(w, locw[c][tb + i + k], cv[i]);
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) convs[tb + i][f] = cv[i];
  }
  __syncthreads();
  const int col = tid;
  float Lr[NF], dLa[NF];
#pragma unroll
  for (int f = 0; f < NF; f += 4) {
    const float4 l = ld4(a.L + (long)col * NF + f);
    Lr[f] = l.x; Lr[f + 1] = l.y; Lr[f + 2] = l.z; Lr[f + 3] = l.w;
  }
#pragma unroll
  for (int f = 0; f < NF; ++f) dLa[f] = 0.f;
  const float qv = a.q[(long)b * DA + col], vv = a.v[col];
  float dqa = 0.f, dva = 0.f;
  for (int t = 0; t < TC; ++t) {
    float g = 0.f;
    if (t < nt) {
      const long o = ((long)b * Tx + t0 + t) * DA + col;
      float x = qv + a.ep[o];
#pragma unroll
      for (int f = 0; f < NF; ++f) x = fmaf(Lr[f], convs[t][f], x);
      const float av = ft_tanh(x);
      g = des[t] * vv * (1.f - av * av);
      a.dep[o] += g;
      dqa += g;
      dva = fmaf(des[t], av, dva);
#pragma unroll
      for (int f = 0; f < NF; ++f) dLa[f] = fmaf(g, convs[t][f], dLa[f]);
    }
    gs[t][col] = g;
  }
  const long slab = (long)b * a.nch + ch;
  a.dqp[slab * DA + col] = dqa;
  a.dvp[slab * DA + col] += dva;
  float* dl = a.dLp + (slab * DA + col) * NF;
#pragma unroll
  for (int f = 0; f < NF; ++f) dl[f] += dLa[f];
  __syncthreads();
  // dloc[t][f] = sum_col g[t][col] L[col][f]: thread -> token tid / 8, filters 4 (tid % 8) .. +3
  const int t = tid >> 3, fg = 4 * (tid & 7);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = 0; c < DA; ++c) {
    const float g = gs[t][c];
    const float4 l = ld4(a.L + (long)c * NF + fg);
    acc.x = fmaf(g, l.x, acc.x); acc.y = fmaf(g, l.y, acc.y); acc.z = fmaf(g, l.z, acc.z); acc.w = fmaf(g, l.w, acc.w);
  }
  if (t < nt) *reinterpret_cast<float4*>(a.dloc + ((long)b * Tx + t0 + t) * NF + fg) = acc;
}

// 3. location conv backward of one chunk; chunk 0 also adds the item's dq slabs
__global__ __launch_bounds__(256) void ft_taco_conv_bwd_kernel(AttBwdArgs a, int s) {
  __shared__ float dl[WIN][NF + 1];
  __shared__ float inw[2][WIN];
  __shared__ float cws[NF][2 * KW + 1];
  __shared__ float part[4][2 * TC];
  const int ch = blockIdx.x, t0 = ch * TC, b = blockIdx.y, tid = threadIdx.x;
  const int Tx = a.Tx, B = a.B;
  if (ch == 0) {
    float v = 0.f;
    for (int c = 0; c < a.nch; ++c) v += a.dqp[((long)b * a.nch + c) * DA + tid];
    a.dq[((long)s * B + b) * DA + tid] = v;
  }
  if (s == 0) return;                                  // step 0 sees a zero location input: nothing flows on
  for (int i = tid; i < WIN * NF; i += 256) {
    const int o = i / NF, f = i % NF, t = t0 - KP + o;
    dl[o][f] = (t >= 0 && t < Tx) ? a.dloc[((long)b * Tx + t) * NF + f] : 0.f;
  }
  load_window(a, s, b, t0, inw);
  for (int i = tid; i < NCW; i += 256) cws[i / (2 * KW)][i % (2 * KW)] = a.cw[i];
  __syncthreads();
  {
    // din[c][t0 + tl] = sum_{f,k} cw[f,c,k] dloc[t0 + tl - k + 15][f]; thread -> (c, tl, quarter of the filters)
    const int c = tid >> 7, tl = (tid >> 2) & 31, fq = 8 * (tid & 3);
    float acc = 0.f;
    for (int k = 0; k < KW; ++k)
#pragma unroll
      for (int f = 0; f < 8; ++f) acc = fmaf(cws[fq + f][c * KW + k], dl[tl + 2 * KP - k][fq + f], acc);
    part[tid & 3][c * TC + tl] = acc;
  }
  // dcw[f,c,k] slab: sum over the chunk's tokens of dloc[t][f] in[c][t + k - 15]
  for (int e = tid; e < NCW; e += 256) {
    const int f = e / (2 * KW), rem = e % (2 * KW), c = rem / KW, k = rem % KW;
    float acc = 0.f;
    for (int tl = 0; tl < TC; ++tl) acc = fmaf(dl[tl + KP][f], inw[c][tl + k], acc);
    a.dcwp[((long)b * a.nch + ch) * NCW + e] += acc;
  }
  __syncthreads();
  if (tid < 2 * TC) {
    const int c = tid >> 5, t = t0 + (tid & 31);
    if (t < Tx) {
      const float v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
      if (c == 0) a.dcum[(long)b * Tx + t] += v;
      else a.dal[(long)b * Tx + t] = v;
    }
  }
}

// 4. GRU cell backward: the forward's gate product again (ft_taco_gru_kernel's tile), then the cell
__global__ __launch_bounds__(256) void ft_taco_gru_bwd_kernel(AttBwdArgs a, int s) {
  __shared__ float red[4][16][17];
  __shared__ float wq[4][16 * UB];
  const int ub = blockIdx.x, u0 = ub * UB, b0 = blockIdx.y * 16;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
  const int B = a.B, S = a.S;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (s > 0) {
    constexpr int KQ = DA / 2;
    const int kh = wave >> 1, k0 = KQ * (wave & 1);
    const int bA = min(b0 + l15, B - 1);
    const float* arow = a.hist + ((long)(s - 1) * B + bA) * 2 * DA + (kh == 0 ? 0 : DA) + k0;
    const int qn = l15 & 3, u = u0 + (l15 >> 2);
    const int g = qn < 2 ? qn : 2;
    const bool zero = (kh == 0 && qn == 3) || (kh == 1 && qn == 2);
    const float* brow = (kh == 0 ? a.wih + (long)(g * DA + u) * a.ld_wih : a.whh + (long)(g * DA + u) * DA) + k0;
    for (int c = 0; c < KQ / 16; ++c) {
      const float4 av = ld4(arow + 16 * c + 4 * q);
      const float4 bv = zero ? make_float4(0.f, 0.f, 0.f, 0.f) : ld4(brow + 16 * c + 4 * q);
      mfma4(av, bv, acc);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[wave][4 * q + e][l15] = acc[e];
  // (W^T dq)[b, u]: thread -> (quarter of i, item, unit)
  {
    const int kq = tid >> 6, r = tid & 63, cb = min(b0 + (r >> 2), B - 1), cu = u0 + (r & 3);
    const float* dq = a.dq + ((long)s * B + cb) * DA;
    float v = 0.f;
    for (int i = 64 * kq; i < 64 * kq + 64; ++i) v = fmaf(dq[i], a.W[(long)i * DA + cu], v);
    wq[kq][r] = v;
  }
  __syncthreads();
  if (tid >= 16 * UB) return;
  const int crow = tid / UB, cj = tid % UB, cb = b0 + crow, cu = u0 + cj;
  if (cb >= B) return;
  const long row = (long)s * B + cb;
  const float* pr = a.P + row * NG;
  const int c0 = 4 * cj;
  const float sr = (red[0][crow][c0] + red[1][crow][c0]) + (red[2][crow][c0] + red[3][crow][c0]);
  const float sz = (red[0][crow][c0 + 1] + red[1][crow][c0 + 1]) + (red[2][crow][c0 + 1] + red[3][crow][c0 + 1]);
  const float nx = red[0][crow][c0 + 2] + red[1][crow][c0 + 2];
  const float nh = red[2][crow][c0 + 3] + red[3][crow][c0 + 3];
  const float r = ft_sigmoid(pr[cu] + sr + a.bhh[cu]);
  const float z = ft_sigmoid(pr[DA + cu] + sz + a.bhh[DA + cu]);
  const float nhb = nh + a.bhh[2 * DA + cu];
  const float n = ft_tanh(pr[2 * DA + cu] + nx + r * nhb);
  const float hp = s > 0 ? a.hist[(row - B) * 2 * DA + DA + cu] : 0.f;
  float dh = a.dhist[row * 2 * DA + DA + cu] + ((wq[0][tid] + wq[1][tid]) + (wq[2][tid] + wq[3][tid]));
  if (s < S - 1) dh += a.dh[(long)cb * DA + cu];
  const float dnp = dh * (1.f - z) * (1.f - n * n);
  const float dzp = dh * (hp - n) * z * (1.f - z);
  const float drp = dnp * nhb * r * (1.f - r);
  float* dp = a.dP + row * NG;
  float* dg = a.dgh + row * NG;
  dp[cu] = drp; dp[DA + cu] = dzp; dp[2 * DA + cu] = dnp;
  dg[cu] = drp; dg[DA + cu] = dzp; dg[2 * DA + cu] = dnp * r;
  a.zdh[(long)cb * DA + cu] = z * dh;
}

// 5. carried terms of step s-1: z = 0: dctx = dgx_s W_ih[:, :256]; z = 1: dh = dgh_s W_hh + z_s dh_s
__global__ __launch_bounds__(256) void ft_taco_carry_kernel(AttBwdArgs a, int s) {
  __shared__ float red[4][16][17];
  const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16, which = blockIdx.z;
  const int tid = threadIdx.x, l15 = tid & 15, B = a.B;
  const float* arow = (which ? a.dgh : a.dP) + ((long)s * B + min(b0 + l15, B - 1)) * NG;
  const float* brow = (which ? a.whhT : a.wihT) + (long)(j0 + l15) * NG;
  const float v = tile16(arow, brow, NG, red);
  const int cb = b0 + (tid >> 4), j = j0 + l15;
  if (cb >= B) return;
  const long o = (long)cb * DA + j;
  if (which) a.dh[o] = v + a.zdh[o];
  else a.dctx[o] = v;
}

// dst[i] = sum_j src[j * n + i], j ascending
__global__ void ft_taco_slab_sum_kernel(const float* __restrict__ src, int nslabs, int n, float* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = 0.f;
  for (int j = 0; j < nslabs; ++j) v += src[(long)j * n + i];
  dst[i] = v;
}

// ---- small pieces ------------------------------------------------------------------------------------------------------
// PreNet layer backward: y = dropout(relu(z), p) as stored (0 where dropped or clipped) -> dz = y > 0 ? dy / (1 - p) : 0
__global__ void ft_relu_dropout_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                           float* __restrict__ dz, long n, float inv_keep) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    dz[i] = y[i] > 0.f ? dy[i] * inv_keep : 0.f;
}

// mel_proj weight gradient: dwp [r * n_mels, L] in the packed order k * n_mels + n -> dw [n_mels * max_r, L] at rows
// n * max_r + k, exact zeros in the rows k >= r the [:, :, :r] slice drops
__global__ void ft_taco_mel_scatter_kernel(const float* __restrict__ dwp, float* __restrict__ dw, int n_mels, int max_r,
                                           int r, int L) {
  const long total = (long)n_mels * max_r * L;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % L);
    const int row = (int)(i / L), n = row / max_r, k = row % max_r;
    dw[i] = k < r ? dwp[((long)k * n_mels + n) * L + c] : 0.f;
  }
}

struct BwdLayout {
  size_t wihT, whhT, cumP, dgh, dq, q, de, dloc, zero0, dcum, dal, dvp, dLp, dcwp, zero1, dctx, dh, zdh, dqp, gemm,
      colsum, total;
};
BwdLayout bwd_layout(int B, int Tx, int S) {
  BwdLayout w;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t f = sizeof(float), nch = (size_t)ft_cdiv(Tx, TC), bt = (size_t)B * Tx, sb = (size_t)S * B;
  size_t o = 0;
  w.wihT = o;  o = al(o + f * DA * NG);
  w.whhT = o;  o = al(o + f * DA * NG);
  w.cumP = o;  o = al(o + f * sb * Tx);
  w.dgh = o;   o = al(o + f * sb * NG);
  w.dq = o;    o = al(o + f * sb * DA);
  w.q = o;     o = al(o + f * B * DA);
  w.de = o;    o = al(o + f * bt);
  w.dloc = o;  o = al(o + f * bt * NF);
  w.zero0 = o;                                   // dcum | dal | dvp | dLp | dcwp: one memset
  w.dcum = o;  o = al(o + f * bt);
  w.dal = o;   o = al(o + f * bt);
  w.dvp = o;   o = al(o + f * B * nch * DA);
  w.dLp = o;   o = al(o + f * B * nch * DA * NF);
  w.dcwp = o;  o = al(o + f * B * nch * NCW);
  w.zero1 = o;
  w.dctx = o;  o = al(o + f * B * DA);
  w.dh = o;    o = al(o + f * B * DA);
  w.zdh = o;   o = al(o + f * B * DA);
  w.dqp = o;   o = al(o + f * B * nch * DA);
  w.gemm = o;
  size_t g = ft_linear_bwd_weight_workspace((int)sb, DA, NG);
  const size_t g2 = ft_linear_bwd_weight_workspace((int)sb, DA, DA);
  if (g2 > g) g = g2;
  o = al(o + g);
  size_t cs = ft_colsum_workspace((int)sb, NG);
  const size_t cs2 = ft_colsum_workspace((int)sb, DA);
  if (cs2 > cs) cs = cs2;
  w.colsum = o; o = al(o + cs);
  w.total = o;
  return w;
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int ft_relu_dropout_bwd(const float* dy, const float* y, float* dz, long n, float p, void* stream) {
  FT_REQUIRE(n >= 0 && p >= 0.f && p < 1.f, "relu_dropout_bwd: n must be >= 0 and p in [0,1)");
  FT_REQUIRE(n == 0 || (dy && y && dz), "relu_dropout_bwd: null operand");
  if (n == 0) return FT_OK;
  hipLaunchKernelGGL(ft_relu_dropout_bwd_kernel, dim3((unsigned)(n < 256L * 1024 ? ft_cdiv(n, 256) : 1024)), dim3(256),
                     0, (hipStream_t)stream, dy, y, dz, n, 1.f / (1.f - p));
  return ft_check_launch("relu_dropout_bwd");
}

int ft_taco_mel_scatter(const float* dwp, float* dw, int n_mels, int max_r, int r, int L, void* stream) {
  FT_REQUIRE(n_mels >= 1 && L >= 1 && r >= 1 && r <= max_r, "taco_mel_scatter: bad dims (n_mels %d, max_r %d, r %d, L %d)",
             n_mels, max_r, r, L);
  FT_REQUIRE(dwp && dw, "taco_mel_scatter: null operand");
  const long total = (long)n_mels * max_r * L;
  hipLaunchKernelGGL(ft_taco_mel_scatter_kernel, dim3((unsigned)(total < 256L * 1024 ? ft_cdiv(total, 256) : 1024)),
                     dim3(256), 0, (hipStream_t)stream, dwp, dw, n_mels, max_r, r, L);
  return ft_check_launch("taco_mel_scatter");
}

size_t ft_taco_lstm_zone_workspace(int B, int L) {
  if (B < 1 || L < 4 || L % 4 != 0) return 0;
  return sizeof(float) * 3 * (size_t)B * L;
}

int ft_taco_lstm_zone_fwd(const float* xp, const float* w_hh, const float* b_hh, float p, uint64_t seed, float* gates,
                          float* c, float* h, int B, int S, int L, void* stream) {
  FT_REQUIRE(B >= 1 && S >= 1, "taco_lstm_zone_fwd: B and S must be >= 1 (got %d, %d)", B, S);
  FT_REQUIRE(L >= 4 && L % 4 == 0, "taco_lstm_zone_fwd: L must be a positive multiple of 4 (got %d)", L);
  FT_REQUIRE(p >= 0.f && p <= 1.f, "taco_lstm_zone_fwd: p must be in [0,1]");
  FT_REQUIRE(xp && w_hh && b_hh && gates && c && h, "taco_lstm_zone_fwd: null operand");
  FT_REQUIRE(al16(w_hh) && al16(h), "taco_lstm_zone_fwd: w_hh and h must be 16-byte aligned");
  ZoneArgs a{xp, w_hh, b_hh, gates, c, h, B, S, L, p, seed};
  const dim3 grid(L / UB, ft_cdiv(B, 16));
  for (int s = 0; s < S; ++s) hipLaunchKernelGGL(ft_lstm_zone_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, s);
  return ft_check_launch("taco_lstm_zone_fwd");
}

int ft_taco_lstm_zone_bwd(const float* dout, const float* gates, const float* c, const float* w_hhT, float p,
                          uint64_t seed, float* dxp, int B, int S, int L, void* ws, size_t ws_bytes, void* stream) {
  FT_REQUIRE(B >= 1 && S >= 1, "taco_lstm_zone_bwd: B and S must be >= 1 (got %d, %d)", B, S);
  FT_REQUIRE(L >= 4 && L % 4 == 0, "taco_lstm_zone_bwd: L must be a positive multiple of 4 (got %d)", L);
  FT_REQUIRE(p >= 0.f && p <= 1.f, "taco_lstm_zone_bwd: p must be in [0,1]");
  FT_REQUIRE(dout && gates && c && w_hhT && dxp, "taco_lstm_zone_bwd: null operand");
  FT_REQUIRE(al16(w_hhT) && al16(dxp), "taco_lstm_zone_bwd: w_hhT and dxp must be 16-byte aligned");
  const size_t need = ft_taco_lstm_zone_workspace(B, L);
  FT_REQUIRE(ws && ws_bytes >= need, "taco_lstm_zone_bwd: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  float* w = (float*)ws;
  ZoneBwdArgs a{dout, gates, c, w_hhT, dxp, w, w + 2 * (size_t)B * L, B, S, L, p, seed};
  const dim3 grid(ft_cdiv(L, 16), ft_cdiv(B, 16));
  for (int s = S - 1; s >= 0; --s)
    hipLaunchKernelGGL(ft_lstm_zone_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, s);
  return ft_check_launch("taco_lstm_zone_bwd");
}

size_t ft_taco_attend_bwd_workspace(int B, int Tx, int S) {
  if (B < 1 || Tx < 1 || Tx > TXMAX || S < 1) return 0;
  return bwd_layout(B, Tx, S).total;
}

int ft_taco_attend_bwd(const float* enc_proj, const float* enc_pq, const float* P, const float* w_ih, long ld_w_ih,
                       const float* w_hh, const float* b_hh, const float* W, const float* b_W, const float* conv_w,
                       const float* L, const float* b_L, const float* v, const float* hist, const float* attn,
                       const float* dhist, float* dep, float* depq, float* dP, float* dw_ih_ctx, float* dw_hh,
                       float* db_hh, float* dW, float* dbW, float* dconv_w, float* dL, float* dbL, float* dv, int B,
                       int Tx, int S, void* ws, size_t ws_bytes, void* stream) {
  FT_REQUIRE(B >= 1, "taco_attend_bwd: B must be >= 1 (got %d)", B);
  FT_REQUIRE(Tx >= 1 && Tx <= TXMAX, "taco_attend_bwd: Tx must be in 1..%d (got %d)", TXMAX, Tx);
  FT_REQUIRE(S >= 1, "taco_attend_bwd: S must be >= 1 (got %d)", S);
  FT_REQUIRE((long)S * B * NG < (1L << 31), "taco_attend_bwd: S * B too large (%d x %d)", S, B);
  FT_REQUIRE(ld_w_ih >= DA && ld_w_ih % 4 == 0, "taco_attend_bwd: ld_w_ih must be a multiple of 4, >= 256");
  FT_REQUIRE(enc_proj && enc_pq && P && w_ih && w_hh && b_hh && W && b_W && conv_w && L && b_L && v && hist && attn &&
                 dhist, "taco_attend_bwd: null operand");
  FT_REQUIRE(dep && depq && dP && dw_ih_ctx && dw_hh && db_hh && dW && dbW && dconv_w && dL && dbL && dv,
             "taco_attend_bwd: null output");
  FT_REQUIRE(al16(enc_pq) && al16(w_ih) && al16(w_hh) && al16(W) && al16(L) && al16(hist) && al16(depq) && al16(dP) &&
                 al16(ws), "taco_attend_bwd: enc_pq, weights, hist, depq, dP and workspace must be 16-byte aligned");
  const BwdLayout wl = bwd_layout(B, Tx, S);
  FT_REQUIRE(ws && ws_bytes >= wl.total, "taco_attend_bwd: workspace too small (%zu < %zu bytes)", ws_bytes, wl.total);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  auto fp = [&](size_t off) { return (float*)(w + off); };
  AttBwdArgs a;
  a.ep = enc_proj; a.epq = enc_pq; a.P = P; a.wih = w_ih; a.ld_wih = ld_w_ih; a.whh = w_hh; a.bhh = b_hh; a.W = W;
  a.bW = b_W; a.cw = conv_w; a.L = L; a.bL = b_L; a.v = v; a.hist = hist; a.attn = attn; a.dhist = dhist;
  a.dep = dep; a.depq = depq; a.dP = dP;
  a.wihT = fp(wl.wihT); a.whhT = fp(wl.whhT); a.cumP = fp(wl.cumP); a.dgh = fp(wl.dgh);
  a.dq = fp(wl.dq); a.q = fp(wl.q); a.de = fp(wl.de); a.dloc = fp(wl.dloc); a.dcum = fp(wl.dcum); a.dal = fp(wl.dal);
  a.dctx = fp(wl.dctx); a.dh = fp(wl.dh); a.zdh = fp(wl.zdh); a.dqp = fp(wl.dqp); a.dvp = fp(wl.dvp);
  a.dLp = fp(wl.dLp); a.dcwp = fp(wl.dcwp);
  a.B = B; a.Tx = Tx; a.S = S; a.nch = ft_cdiv(Tx, TC);
  const size_t btd = sizeof(float) * (size_t)B * Tx * DA;
  (void)hipMemsetAsync(dep, 0, btd, st);
  (void)hipMemsetAsync(depq, 0, btd, st);
  (void)hipMemsetAsync(w + wl.zero0, 0, wl.zero1 - wl.zero0, st);
  hipLaunchKernelGGL(ft_taco_transpose_kernel, dim3(256), dim3(256), 0, st, w_ih, ld_w_ih, NG, DA, a.wihT);
  hipLaunchKernelGGL(ft_taco_transpose_kernel, dim3(256), dim3(256), 0, st, w_hh, (long)DA, NG, DA, a.whhT);
  hipLaunchKernelGGL(ft_taco_cumprefix_kernel, dim3(ft_cdiv((long)B * Tx, 256)), dim3(256), 0, st, a);
  const int tiles = ft_cdiv(B, 16);
  const dim3 g1(B), g2(a.nch, B), g4(DA / UB, tiles), g5(DA / 16, tiles, 2);
  for (int s = S - 1; s >= 0; --s) {
    hipLaunchKernelGGL(ft_taco_softmax_bwd_kernel, g1, dim3(256), 0, st, a, s);
    hipLaunchKernelGGL(ft_taco_energy_bwd_kernel, g2, dim3(256), 0, st, a, s);
    hipLaunchKernelGGL(ft_taco_conv_bwd_kernel, g2, dim3(256), 0, st, a, s);
    hipLaunchKernelGGL(ft_taco_gru_bwd_kernel, g4, dim3(256), 0, st, a, s);
    if (s > 0) hipLaunchKernelGGL(ft_taco_carry_kernel, g5, dim3(256), 0, st, a, s);
  }
  const int nsl = B * a.nch;
  hipLaunchKernelGGL(ft_taco_slab_sum_kernel, dim3(1), dim3(256), 0, st, a.dvp, nsl, DA, dv);
  hipLaunchKernelGGL(ft_taco_slab_sum_kernel, dim3(DA * NF / 256), dim3(256), 0, st, a.dLp, nsl, DA * NF, dL);
  hipLaunchKernelGGL(ft_taco_slab_sum_kernel, dim3(ft_cdiv(NCW, 256)), dim3(256), 0, st, a.dcwp, nsl, NCW, dconv_w);
  int rc = ft_check_launch("taco_attend_bwd");
  if (rc) return rc;
  const int rows = S * B;
  void* gws = w + wl.gemm;
  const size_t gbytes = wl.colsum - wl.gemm, cbytes = wl.total - wl.colsum;
  // dW_hh = sum_s dgh_s^T h_{s-1}; dW_ih[:, :256] = sum_s dgx_s^T ctx_{s-1}; dW = sum_s dq_s^T h_s
  if ((rc = ft_linear_bwd_weight(a.dgh, NG, hist + DA, 2 * DA, dw_hh, rows, DA, NG, B, S, -1, 0, 1, 1, gws, gbytes, stream)))
    return rc;
  if ((rc = ft_linear_bwd_weight(dP, NG, hist, 2 * DA, dw_ih_ctx, rows, DA, NG, B, S, -1, 0, 1, 1, gws, gbytes, stream)))
    return rc;
  if ((rc = ft_linear_bwd_weight(a.dq, DA, hist + DA, 2 * DA, dW, rows, DA, DA, 1, rows, 0, 0, 0, 0, gws, gbytes, stream)))
    return rc;
  if ((rc = ft_colsum(a.dgh, NG, db_hh, rows, NG, 1.f, 0, w + wl.colsum, cbytes, stream))) return rc;
  if ((rc = ft_colsum(a.dq, DA, dbW, rows, DA, 1.f, 0, w + wl.colsum, cbytes, stream))) return rc;
  (void)hipMemcpyAsync(dbL, dbW, sizeof(float) * DA, hipMemcpyDeviceToDevice, st);
  return ft_check_launch("taco_attend_bwd");
}

}  // extern "C"
