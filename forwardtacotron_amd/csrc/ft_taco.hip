// Tacotron teacher-forced attention recurrence for gfx950 (models/tacotron.py: Decoder.attn_rnn, LSA, context).
//
// Under teacher forcing the recurrence is closed over {h_attn, context, cumulative, attention}: the prenet and the
// prenet half of the GRU input projection are known for all S steps in advance (P [S,B,768], b_ih included), and
// nothing from the decoder LSTMs feeds back.  What is left per step is a fixed chain of three launches:
//
//   1. ft_taco_gru_kernel      grid (256/UB unit blocks, ceil(B/16) batch tiles), 256 threads
//        GRUCell (gates r, z, n; h' = (1-z) n + z h) for 16 items x UB = 4 hidden units.  The 16 x 16 product
//        [context | h] (K = 512) x [4 units x (r, z, n_ctx, n_h)] runs on v_mfma_f32_16x16x4_f32, K split over the
//        four waves (the context half against W_ih[:, :256], the h half against W_hh); the r and z columns add both
//        halves, the n gate keeps them apart (n = tanh(n_x + n_ctx + r * (n_h + b_hn))).  The 768 x 512 weights are
//        spread over the 64 unit blocks, so each step reads them once per batch tile chip-wide.  The workgroup then
//        forms its share of the LSA query, qp[ub][b][:] = W[:, u0:u0+UB] h'[b, u0:u0+UB] (no cross-workgroup
//        reduction: the next kernel sums the 64 slabs in a fixed order, so the result does not depend on scheduling).
//   2. ft_taco_energy_kernel   grid (ceil(Tx/TC) token chunks, B, 4 column quarters), 256 threads
//        q = b_W + b_L + sum of the 64 slabs (the quarter's 64 columns); location conv (2 -> 32 filters, k = 31, zero
//        padding at 0 and Tx) of [cumulative, attention] on the VALU into LDS; the [TC x 32] x [32 x 64] projection L
//        on MFMA; per token the partial energy v . tanh(q + enc_proj + L conv) over the quarter's columns (hardware
//        exp / rcp tanh, |error| <= ~2e-7 per term).
//   3. ft_taco_context_kernel  grid (8 column chunks, B), 256 threads
//        energies = sum of the 4 partials; softmax over all Tx columns (no mask, like the reference; with
//        AttendArgs.lens over the item's own tokens, see the ragged-batch section below); chunk 0 writes attn[b, s, :], attention := p and
//        cumulative += p; every chunk forms 32 columns of context = p @ enc_pq (each recomputes the softmax from the
//        Tx energies, so no chunk waits for another).
// Each kernel requests all of its global operands before its first dependent use: a step costs three launches and
// one memory round trip per launch.
//
// Every sum runs in a fixed order and no atomics are used: the same inputs give the same bits, whether the call
// keeps the histories (forward) or not (align).  The LSA state (cumulative, attention) lives in the workspace for the
// duration of the call.  All arithmetic is fp32 (the f32 MFMA products are exact fp32).
#include "ft_common.h"
#include "fwdtaco_hip.h"

namespace {

constexpr int DA = 256;          // decoder / attention dims (the reference runs with no other value)
constexpr int NG = 3 * DA;       // GRU gate rows
constexpr int NF = 32;           // location filters
constexpr int KW = 31;           // location kernel width (padding 15)
constexpr int KP = KW / 2;
constexpr int UB = 4;            // hidden units per GRU workgroup
constexpr int NUB = DA / UB;     // query partial slabs
constexpr int TC = 32;           // tokens per energy workgroup
constexpr int NCQ = 4;           // attention-column quarters per energy workgroup grid (partial energies)
constexpr int NAC = 8;           // context column chunks per item
constexpr int TXMAX = 1024;
constexpr int CLD = NF + 4;      // LDS row stride of the conv outputs (16-B aligned rows)

struct AttendArgs {
  const float* enc_proj;   // [B,Tx,256]
  const float* enc_pq;     // [B,Tx,256]
  const float* P;          // [S,B,768]
  const float* wih;        // [768, ld_wih]: context columns 0..255
  long ld_wih;
  const float* whh;        // [768,256]
  const float* bhh;        // [768]
  const float* W;          // [256,256]
  const float* bW;         // [256]
  const float* cw;         // [32,2,31]
  const float* L;          // [256,32]
  const float* bL;         // [256]
  const float* v;          // [256]
  float* attn;             // [B,S,Tx]
  float* qp;               // [NUB,B,256]
  float* E;                // [B,NCQ,Tx] partial energies
  float* cum;              // [B,Tx]
  float* att;              // [B,Tx]
  int B, Tx, S;
  long ldh;                // row stride (floats) of the h / context state rows
  const long* lens;        // [B] valid tokens per item (ragged batch), or nullptr: every item has Tx
};

// valid tokens of item b: the energies, the softmax, the LSA state and the context stop there
__device__ __forceinline__ int item_len(const AttendArgs& a, int b) {
  return a.lens ? (int)min(max(a.lens[b], 1L), (long)a.Tx) : a.Tx;
}

__device__ __forceinline__ void mfma4(const float4& a, const float4& b, f32x4& acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

// f32 16x16x4 operand convention used below: lane (i = lane & 15, q = lane >> 4) holds row i, k = 16c + 4q .. +3 of
// both operands; the accumulator holds D[4q + e][i].

// ---- 1. GRUCell + query partials ------------------------------------------------------------------------------------
// 16 columns = UB (4) units x (r, z, n from the context, n from h); the four waves split K = 512 into quarters (waves
// 0, 1: the context half against W_ih[:, :256]; waves 2, 3: the h half against W_hh), so a wave moves 8 KB of each
// operand and issues 32 MFMAs.
__global__ __launch_bounds__(256) void ft_taco_gru_kernel(AttendArgs a, int s, const float* __restrict__ hprev,
                                                           const float* __restrict__ cprev, float* __restrict__ hout) {
  __shared__ float red[4][16][17];
  __shared__ float hs[16][UB];
  const int ub = blockIdx.x, u0 = ub * UB, b0 = blockIdx.y * 16;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
  const int B = a.B;

  // cell operands (requested before the matmul): thread tid < 16 * UB owns item b0 + tid / UB, unit u0 + tid % UB
  const int crow = tid / UB, cj = tid % UB, cb = b0 + crow, cu = u0 + cj;
  const bool cact = tid < 16 * UB && cb < B;
  float xr = 0.f, xz = 0.f, xn = 0.f, br = 0.f, bz = 0.f, bn = 0.f, hp = 0.f;
  if (cact) {
    const float* pr = a.P + ((long)s * B + cb) * NG;
    xr = pr[cu]; xz = pr[DA + cu]; xn = pr[2 * DA + cu];
    br = a.bhh[cu]; bz = a.bhh[DA + cu]; bn = a.bhh[2 * DA + cu];
    if (s > 0) hp = hprev[(long)cb * a.ldh + cu];
  }
  // query-partial weights of this thread's row (consumed at the end): requested with the matmul operands
  const float4 w0 = *reinterpret_cast<const float4*>(a.W + (long)tid * DA + u0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (s > 0) {                          // step 0: h = context = 0, the products vanish
    constexpr int KQ = DA / 2;          // K per wave
    const int kh = wave >> 1, k0 = KQ * (wave & 1);
    const int bA = min(b0 + l15, B - 1);          // rows past B read item B-1 and are never consumed
    const float* arow = (kh == 0 ? cprev : hprev) + (long)bA * a.ldh + k0;
    const int qn = l15 & 3, u = u0 + (l15 >> 2);
    const int g = qn < 2 ? qn : 2;
    const bool zero = (kh == 0 && qn == 3) || (kh == 1 && qn == 2);
    const float* brow = (kh == 0 ? a.wih + (long)(g * DA + u) * a.ld_wih : a.whh + (long)(g * DA + u) * DA) + k0;
    // the wave's whole K slice of both operands is requested before the first MFMA: one memory round trip
    float4 av[KQ / 16], bv[KQ / 16];
#pragma unroll
    for (int c = 0; c < KQ / 16; ++c) {
      av[c] = *reinterpret_cast<const float4*>(arow + 16 * c + 4 * q);
      bv[c] = *reinterpret_cast<const float4*>(brow + 16 * c + 4 * q);
    }
#pragma unroll
    for (int c = 0; c < KQ / 16; ++c) mfma4(av[c], zero ? make_float4(0.f, 0.f, 0.f, 0.f) : bv[c], acc);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[wave][4 * q + e][l15] = acc[e];
  __syncthreads();

  if (tid < 16 * UB) {
    float h = 0.f;
    if (cact) {
      const int c0 = 4 * cj;
      const float sr = (red[0][crow][c0] + red[1][crow][c0]) + (red[2][crow][c0] + red[3][crow][c0]);
      const float sz = (red[0][crow][c0 + 1] + red[1][crow][c0 + 1]) + (red[2][crow][c0 + 1] + red[3][crow][c0 + 1]);
      const float nx = red[0][crow][c0 + 2] + red[1][crow][c0 + 2];
      const float nh = red[2][crow][c0 + 3] + red[3][crow][c0 + 3];
      const float r = ft_sigmoid(xr + sr + br);
      const float z = ft_sigmoid(xz + sz + bz);
      const float n = ft_tanh(xn + nx + r * (nh + bn));
      h = (1.f - z) * n + z * hp;
      hout[(long)cb * a.ldh + cu] = h;
    }
    hs[crow][cj] = h;
  }
  __syncthreads();

  // query partial of this unit block: qp[ub][b][i] = sum_j W[i, u0 + j] h'[b, u0 + j]
  const int i = tid;
  for (int row = 0; row < 16 && b0 + row < B; ++row) {
    const float* hr = hs[row];
    float v = w0.x * hr[0];
    v = fmaf(w0.y, hr[1], v); v = fmaf(w0.z, hr[2], v); v = fmaf(w0.w, hr[3], v);
    a.qp[((long)ub * B + b0 + row) * DA + i] = v;
  }
}

// ---- 2. LSA energies --------------------------------------------------------------------------------------------------
// Workgroup = (TC tokens, item, NCQ-th of the 256 attention columns): it writes the partial energy of its 64 columns,
// E[b][cq][t]; the context kernel adds the NCQ partials.  Every global operand of the workgroup (its columns of the 64
// query slabs, the location window, the conv weights, its L rows, enc_proj at the lane's positions) is requested at
// the top, so the kernel pays one memory round trip; the phases after it run from registers and LDS.
__global__ __launch_bounds__(256) void ft_taco_energy_kernel(AttendArgs a) {
  constexpr int NT = TC / 16;
  constexpr int WIN = TC + KW - 1;
  constexpr int CQ = DA / NCQ;                    // 64 columns: one 16-column tile per wave
  constexpr int SG = 256 / CQ;                    // slab groups of the query sum
  __shared__ float qsum[SG][CQ];
  __shared__ float locw[2][WIN];
  __shared__ float cws[NF][2 * KW + 1];           // odd row stride: the 32 filters of a wave hit 32 banks
  __shared__ __attribute__((aligned(16))) float convs[TC][CLD];
  __shared__ float esum[4][TC];
  const int t0 = blockIdx.x * TC, b = blockIdx.y, cq = blockIdx.z;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
  const int B = a.B, Tx = a.Tx;
  const int n = item_len(a, b);
  if (t0 >= n) return;                            // every token of the chunk is padding: nothing to store
  const int col = CQ * cq + 16 * wave + l15;      // this lane's attention column in the MFMA / energy phases

  float qv[NUB / SG];
  {
    const int qc = CQ * cq + tid % CQ, sg = tid / CQ;
#pragma unroll
    for (int j = 0; j < NUB / SG; ++j) qv[j] = a.qp[((long)(sg * (NUB / SG) + j) * B + b) * DA + qc];
  }
  for (int i = tid; i < 2 * WIN; i += 256) {
    const int c = i / WIN, o = i - c * WIN, t = t0 - KP + o;
    locw[c][o] = (t >= 0 && t < n) ? (c == 0 ? a.cum : a.att)[(long)b * Tx + t] : 0.f;
  }
  for (int i = tid; i < NF * 2 * KW; i += 256) cws[i / (2 * KW)][i % (2 * KW)] = a.cw[i];
  // L row of the lane's column (MFMA B operand): k = 16c + 4q .. +3
  float4 bv[NF / 16];
#pragma unroll
  for (int c = 0; c < NF / 16; ++c) bv[c] = *reinterpret_cast<const float4*>(a.L + (long)col * NF + 16 * c + 4 * q);
  const float qb = a.bW[col] + a.bL[col], vv = a.v[col];
  // enc_proj at the lane's accumulator positions: tokens 16tt + 4q + e
  float epv[NT][4];
#pragma unroll
  for (int tt = 0; tt < NT; ++tt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int t = t0 + 16 * tt + 4 * q + e;
      epv[tt][e] = a.enc_proj[((long)b * Tx + min(t, n - 1)) * DA + col];
    }
  {
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < NUB / SG; ++j) v += qv[j];
    qsum[tid / CQ][tid % CQ] = v;
  }
  __syncthreads();

  // location conv: thread -> filter tid % 32, tokens 4 (tid / 32) .. +3, window held in registers
  {
    const int f = tid & 31, tb = 4 * (tid >> 5);
    float cv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float win[4 + KW - 1];
#pragma unroll
      for (int j = 0; j < 4 + KW - 1; ++j) win[j] = locw[c][tb + j];
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        const float w = cws[f][c * KW + k];
#pragma unroll
        for (int i = 0; i < 4; ++i) cv[i] = fmaf(w, win[i + k], cv[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) convs[tb + i][f] = cv[i];
  }
  __syncthreads();

  // L projection on MFMA: [TC tokens x 32 filters] x [32 x the wave's 16 columns]
  f32x4 acc[NT];
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NF / 16; ++c)
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
      mfma4(*reinterpret_cast<const float4*>(&convs[16 * tt + l15][16 * c + 4 * q]), bv[c], acc[tt]);

  // partial energies: v . tanh(q + enc_proj + L conv) over the 16 column lanes, then over the 4 waves
  const int lc = 16 * wave + l15;
  float qcol = qb;
#pragma unroll
  for (int g = 0; g < SG; ++g) qcol += qsum[g][lc];
#pragma unroll
  for (int tt = 0; tt < NT; ++tt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float sum = vv * ft_tanh_fast(qcol + epv[tt][e] + acc[tt][e]);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
      if (l15 == 0) esum[wave][16 * tt + 4 * q + e] = sum;
    }
  __syncthreads();
  if (tid < TC && t0 + tid < n)
    a.E[((long)b * NCQ + cq) * Tx + t0 + tid] = ((esum[0][tid] + esum[1][tid]) + esum[2][tid]) + esum[3][tid];
}

// ---- 3. softmax, LSA state, context ---------------------------------------------------------------------------------
__device__ __forceinline__ float block_max(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ float block_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void ft_taco_context_kernel(AttendArgs a, int s, float* __restrict__ cout) {
  constexpr int CC = DA / NAC;               // context columns per workgroup
  constexpr int TG = 256 / CC;               // token groups
  constexpr int PF = 24;                     // enc_pq values per thread requested before the softmax (Tx <= PF * TG)
  __shared__ float p[TXMAX];
  __shared__ float red[256];
  __shared__ float sh[4];
  const int ac = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int Tx = a.Tx, n = item_len(a, b);
  const int col = CC * ac + tid % CC, tg = tid / CC;
  const float* pq = a.enc_pq + (long)b * Tx * DA + col;
  float xv[PF];
#pragma unroll
  for (int j = 0; j < PF; ++j) {
    const int t = tg + TG * j;
    xv[j] = t < n ? pq[(long)t * DA] : 0.f;
  }
  const float* e = a.E + (long)b * NCQ * Tx;
  float m = -INFINITY;
  for (int t = tid; t < n; t += 256) {
    const float v = (e[t] + e[Tx + t]) + (e[2 * Tx + t] + e[3 * Tx + t]);
    p[t] = v;
    m = fmaxf(m, v);
  }
  m = block_max(m, sh);
  float z = 0.f;
  for (int t = tid; t < n; t += 256) {
    const float x = expf(p[t] - m);
    p[t] = x;
    z += x;
  }
  z = block_sum(z, sh);              // (its barriers also order the p[] writes above before the reads below)
  for (int t = tid; t < n; t += 256) {
    const float x = p[t] / z;
    p[t] = x;
    if (ac == 0) {
      const long o = (long)b * Tx + t;
      a.attn[((long)b * a.S + s) * Tx + t] = x;
      a.att[o] = x;
      a.cum[o] += x;
    }
  }
  if (ac == 0)                        // ragged batch: exact zeros past the item's tokens
    for (int t = n + tid; t < Tx; t += 256) a.attn[((long)b * a.S + s) * Tx + t] = 0.f;
  __syncthreads();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < PF; ++j) {
    const int t = tg + TG * j;
    if (t < n) acc[j & 3] = fmaf(p[t], xv[j], acc[j & 3]);
  }
  int t = tg + TG * PF;
  for (; t + 3 * TG < n; t += 4 * TG) {
    float x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = pq[(long)(t + i * TG) * DA];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = fmaf(p[t + i * TG], x[i], acc[i]);
  }
  for (; t < n; t += TG) acc[0] = fmaf(p[t], pq[(long)t * DA], acc[0]);
  red[tid] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  if (tid < CC) {
    float v = 0.f;
#pragma unroll
    for (int g = 0; g < TG; ++g) v += red[g * CC + tid];
    cout[(long)b * a.ldh + col] = v;
  }
}

// ---- teacher-forced prenet input frames -----------------------------------------------------------------------------
__global__ void ft_taco_frames_kernel(const float* __restrict__ mel, int n_mels, int Tm, int r, int S, int B,
                                      float* __restrict__ out) {
  const long n = (long)S * B * n_mels;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % n_mels);
    const long sb = i / n_mels;
    const int b = (int)(sb % B), st = (int)(sb / B);
    float v = 0.f;
    if (st > 0) v = mel[((long)b * n_mels + c) * Tm + (long)st * r - 1];
    out[i] = v;
  }
}

__global__ void ft_taco_add_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out,
                                   long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = x[i] + y[i];
}

struct WsLayout {
  size_t qp, E, cum, att, zero, ring, total;
};
WsLayout ws_layout(int B, int Tx) {
  WsLayout w;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t o = 0;
  w.qp = o;   o = al(o + sizeof(float) * (size_t)NUB * B * DA);
  w.E = o;    o = al(o + sizeof(float) * (size_t)B * NCQ * Tx);
  w.cum = o;  o = al(o + sizeof(float) * (size_t)B * Tx);       // cum | att | zero: one memset
  w.att = o;  o = al(o + sizeof(float) * (size_t)B * Tx);
  w.zero = o; o = al(o + sizeof(float) * (size_t)B * 2 * DA);
  w.ring = o; o = al(o + sizeof(float) * (size_t)2 * B * 2 * DA);   // [parity][B][context | h] when no history
  w.total = o;
  return w;
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

size_t ft_taco_attend_workspace(int B, int Tx) {
  if (B < 1 || Tx < 1 || Tx > TXMAX) return 0;
  return ws_layout(B, Tx).total;
}

int ft_taco_attend(const float* enc_proj, const float* enc_pq, const float* P, const float* w_ih, long ld_w_ih,
                   const float* w_hh, const float* b_hh, const float* W, const float* b_W, const float* conv_w,
                   const float* L, const float* b_L, const float* v, float* attn, float* hist, int B, int Tx, int S,
                   void* ws, size_t ws_bytes, void* stream) {
  FT_REQUIRE(B >= 1, "taco_attend: B must be >= 1 (got %d)", B);
  FT_REQUIRE(Tx >= 1 && Tx <= TXMAX, "taco_attend: Tx must be in 1..%d (got %d)", TXMAX, Tx);
  FT_REQUIRE(S >= 1, "taco_attend: S must be >= 1 (got %d)", S);
  FT_REQUIRE(ld_w_ih >= DA && ld_w_ih % 4 == 0, "taco_attend: ld_w_ih must be a multiple of 4, >= 256");
  FT_REQUIRE(enc_proj && enc_pq && P && w_ih && w_hh && b_hh && W && b_W && conv_w && L && b_L && v && attn,
             "taco_attend: null operand");
  FT_REQUIRE(al16(w_ih) && al16(w_hh) && al16(W) && al16(L) && al16(hist) && al16(ws),
             "taco_attend: weights, history and workspace must be 16-byte aligned");
  const WsLayout wl = ws_layout(B, Tx);
  FT_REQUIRE(ws && ws_bytes >= wl.total, "taco_attend: workspace too small (%zu < %zu bytes)", ws_bytes, wl.total);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  AttendArgs a;
  a.enc_proj = enc_proj; a.enc_pq = enc_pq; a.P = P; a.wih = w_ih; a.ld_wih = ld_w_ih; a.whh = w_hh; a.bhh = b_hh;
  a.W = W; a.bW = b_W; a.cw = conv_w; a.L = L; a.bL = b_L; a.v = v; a.attn = attn;
  a.qp = (float*)(w + wl.qp); a.E = (float*)(w + wl.E); a.cum = (float*)(w + wl.cum); a.att = (float*)(w + wl.att);
  a.B = B; a.Tx = Tx; a.S = S;
  a.ldh = 2 * DA; a.lens = nullptr;
  float* zero = (float*)(w + wl.zero);
  float* ring = (float*)(w + wl.ring);
  (void)hipMemsetAsync(w + wl.cum, 0, wl.ring - wl.cum, st);
  const long slab = (long)B * 2 * DA;     // one step of [context | h] rows
  auto state = [&](int step) -> float* { return hist ? hist + step * slab : ring + (step & 1) * slab; };
  const dim3 g1(NUB, ft_cdiv(B, 16)), g2(ft_cdiv(Tx, TC), B, NCQ), g3(NAC, B);
  for (int s = 0; s < S; ++s) {
    const float* prev = s == 0 ? zero : state(s - 1);
    float* cur = state(s);
    hipLaunchKernelGGL(ft_taco_gru_kernel, g1, dim3(256), 0, st, a, s, prev + DA, prev, cur + DA);
    hipLaunchKernelGGL(ft_taco_energy_kernel, g2, dim3(256), 0, st, a);
    hipLaunchKernelGGL(ft_taco_context_kernel, g3, dim3(256), 0, st, a, s, cur);
  }
  return ft_check_launch("taco_attend");
}

int ft_taco_frames(const float* mel, int B, int n_mels, int Tm, int r, int S, float* out, void* stream) {
  FT_REQUIRE(B >= 1 && n_mels >= 1 && r >= 1 && S >= 1, "taco_frames: bad dims");
  FT_REQUIRE((long)(S - 1) * r - 1 < Tm, "taco_frames: step %d reads frame %ld of %d", S - 1, (long)(S - 1) * r - 1, Tm);
  const long n = (long)S * B * n_mels;
  hipLaunchKernelGGL(ft_taco_frames_kernel, dim3((unsigned)(n < 256L * 1024 ? ft_cdiv(n, 256) : 1024)), dim3(256), 0,
                     (hipStream_t)stream, mel, n_mels, Tm, r, S, B, out);
  return ft_check_launch("taco_frames");
}

int ft_taco_add(const float* x, const float* y, float* out, long n, void* stream) {
  FT_REQUIRE(n >= 0, "taco_add: bad size");
  if (n == 0) return FT_OK;
  hipLaunchKernelGGL(ft_taco_add_kernel, dim3((unsigned)(n < 256L * 1024 ? ft_cdiv(n, 256) : 1024)), dim3(256), 0,
                     (hipStream_t)stream, x, y, out, n);
  return ft_check_launch("taco_add");
}

}  // extern "C"

// =====================================================================================================================
// Autoregressive generate (models/tacotron.py:283-349 Tacotron.generate, B = 1, eval mode).
//
// Step s reads the last frame step s-1 produced, so the prenet, the decoder LSTMs and mel_proj move inside the
// recurrence.  Each step is a fixed chain of eight launches; ft_taco_gen_steps enqueues every one from C:
//
//   1. ft_taco_gen_prenet_kernel  grid 24, 1024 threads: frame s*r - 1 (zeros at s = 0) -> fc1 + ReLU (four threads
//        per row) -> fc2 + ReLU (wave per row) -> P[s] = W_ih[:, 256:] p + b_ih, 32 of the 768 rows per workgroup
//        (each workgroup recomputes the 80 -> 256 -> 128 prenet: L2 reads instead of two more launches).
//   2-4. ft_taco_gru_kernel, ft_taco_energy_kernel, ft_taco_context_kernel, unchanged (B = 1, AttendArgs.S = S):
//        hist[s] = [context | h_attn], attn[0, s, :].
//   5. ft_taco_gen_rnnin_kernel   grid ceil(L/4): xin = Wi hist[s] + bi, one wave per output row.
//   6, 7. ft_taco_gen_lstm_kernel grid ceil(L/4): one LSTMCell step per wave and hidden unit (its 4 gate rows of W_ih
//        and W_hh, gate order i, f, g, o), then the residual add x + h'.  h and c ping-pong on the parity of s.
//   8. ft_taco_gen_mel_kernel     grid ceil(80 r/4): mel_proj rows n*20 + k (k < r, the [:, :, :r] slice), one wave
//        per row -> frames[s*r + k][n] (channels last); the stop test (every value < stop_threshold, s*r > 10) is an
//        OR of per-workgroup "not below" flags, read by the last workgroup to finish (a ticket counter: the atomics
//        count and flag, they never carry values), which records S_out = s + 1 the first time the test holds.
//
// Dot products run one wave per row: each lane accumulates k = 4 lane + 256 c .. +3 in ascending c, then a fixed xor
// butterfly sums the 64 lanes (every lane ends with the same bits).  At lstm_dims = 512 the chunk count is a template
// constant and every load of a wave is issued before its first FMA; other sizes take the same order in a loop.
// Steps past the stop still run when they were already enqueued; they write slots past S_out only.
namespace {

constexpr int GNM = 80;          // n_mels (the reference runs with no other value)
constexpr int GF1 = 256;         // prenet fc1
constexpr int GF2 = 128;         // prenet fc2
constexpr int GMAXR = 20;        // Decoder.max_r
constexpr int GPB = 24;          // prenet workgroups (NG / GPB rows of P each)

struct GenArgs {
  const float *fc1w, *fc1b, *fc2w, *fc2b;     // [256,80] [256] [128,256] [128]
  const float* wih;                           // attn_rnn.weight_ih [768, ld_wih]: prenet columns 256..383
  long ld_wih;
  const float* bih;                           // [768]
  const float *wi, *bi;                       // rnn_input [L,512] [L]
  const float *l1ih, *l1hh, *l1bih, *l1bhh;   // res_rnn1 [4L,L] [4L,L] [4L] [4L]
  const float *l2ih, *l2hh, *l2bih, *l2bhh;   // res_rnn2
  const float* wmel;                          // mel_proj [1600, L]
  float thr;
  float* P;         // [S,768]
  float* hist;      // [S,512]
  float* frames;    // [S*r,80]
  int* sout;
  float *xin, *x1, *x2;         // [L]
  float *h1, *c1, *h2, *c2;     // [2][L]
  unsigned *flag, *ticket;
  int L, r, S;
};

__device__ __forceinline__ float wave_allsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float fma4(const float4& a, const float4& b, float acc) {
  acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}

// NR dot products of length K, one wave: out[i] = w[i] . v[i], the same bits in every lane.  KC > 0: K == 256 KC.
template <int NR, int KC>
__device__ __forceinline__ void wave_dots(const float* const (&w)[NR], const float* const (&v)[NR], int K,
                                          float (&out)[NR]) {
  const int lane = threadIdx.x & 63;
  float acc[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) acc[i] = 0.f;
  if constexpr (KC > 0) {
    float4 a[NR][KC], b[NR][KC];
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        a[i][c] = ld4(w[i] + 256 * c + 4 * lane);
        b[i][c] = ld4(v[i] + 256 * c + 4 * lane);
      }
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
      for (int c = 0; c < KC; ++c) acc[i] = fma4(a[i][c], b[i][c], acc[i]);
  } else if ((K & 3) == 0) {
    for (int k = 4 * lane; k < K; k += 256) {
      float4 a[NR], b[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) { a[i] = ld4(w[i] + k); b[i] = ld4(v[i] + k); }
#pragma unroll
      for (int i = 0; i < NR; ++i) acc[i] = fma4(a[i], b[i], acc[i]);
    }
  } else {
    for (int k0 = 4 * lane; k0 < K; k0 += 256)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + e;
        if (k < K) {
#pragma unroll
          for (int i = 0; i < NR; ++i) acc[i] = fmaf(w[i][k], v[i][k], acc[i]);
        }
      }
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) out[i] = wave_allsum(acc[i]);
}

// ---- 1. decoder prenet + prenet half of the GRU input projection ----------------------------------------------------
// 16 waves.  Every weight the workgroup reads (a quarter row of fc1 per thread, 8 fc2 rows per wave, 2 rows of
// W_ih[:, 256:] per wave) is requested with the frame, so the three dependent products cost one memory round trip.
__global__ __launch_bounds__(1024) void ft_taco_gen_prenet_kernel(GenArgs g, int s) {
  constexpr int RPB = NG / GPB;                 // P rows per workgroup
  constexpr int RPW = RPB / 16;                 // per wave
  constexpr int R2 = GF2 / 16;                  // fc2 rows per wave
  constexpr int KQ = GNM / 4;                   // fc1 K quarter
  static_assert(RPW * 16 == RPB && R2 * 16 == GF2 && GF2 == 128 && GF1 == 256 && KQ % 4 == 0, "prenet shape");
  __shared__ __attribute__((aligned(16))) float f[GNM];
  __shared__ float part[4][GF1];
  __shared__ __attribute__((aligned(16))) float p1[GF1];
  __shared__ __attribute__((aligned(16))) float p2[GF2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (s == 0 && blockIdx.x == 0 && tid == 0) *g.sout = g.S;
  const int row1 = tid & (GF1 - 1), q1 = tid >> 8;
  float4 w1[KQ / 4];
#pragma unroll
  for (int c = 0; c < KQ / 4; ++c) w1[c] = ld4(g.fc1w + (long)row1 * GNM + KQ * q1 + 4 * c);
  float4 w2[R2];
#pragma unroll
  for (int i = 0; i < R2; ++i) w2[i] = ld4(g.fc2w + (long)(wave * R2 + i) * GF1 + 4 * lane);
  const int r3 = blockIdx.x * RPB + wave * RPW;
  float4 w3[RPW];
#pragma unroll
  for (int i = 0; i < RPW; ++i)
    w3[i] = lane < GF2 / 4 ? ld4(g.wih + (long)(r3 + i) * g.ld_wih + DA + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float b1 = g.fc1b[row1];
  const float b2 = lane < R2 ? g.fc2b[wave * R2 + lane] : 0.f;
  const float b3 = lane < RPW ? g.bih[r3 + lane] : 0.f;
  if (tid < GNM) f[tid] = s > 0 ? g.frames[((long)s * g.r - 1) * GNM + tid] : 0.f;
  __syncthreads();
  {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < KQ / 4; ++c) acc = fma4(w1[c], ld4(f + KQ * q1 + 4 * c), acc);
    part[q1][row1] = acc;
  }
  __syncthreads();
  if (tid < GF1) p1[tid] = fmaxf(((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid] + b1, 0.f);
  __syncthreads();
  {
    const float4 v = ld4(p1 + 4 * lane);
    float o = 0.f;
#pragma unroll
    for (int i = 0; i < R2; ++i) {
      const float d = wave_allsum(fma4(w2[i], v, 0.f));
      o = lane == i ? d : o;
    }
    if (lane < R2) p2[wave * R2 + lane] = fmaxf(o + b2, 0.f);
  }
  __syncthreads();
  {
    const float4 v = lane < GF2 / 4 ? ld4(p2 + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
    float o = 0.f;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const float d = wave_allsum(fma4(w3[i], v, 0.f));
      o = lane == i ? d : o;
    }
    if (lane < RPW) g.P[(long)s * NG + r3 + lane] = o + b3;
  }
}

// ---- 5. rnn_input ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ft_taco_gen_rnnin_kernel(GenArgs g, int s) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= g.L) return;
  const float* w[1] = {g.wi + (long)j * 2 * DA};
  const float* v[1] = {g.hist + (long)s * 2 * DA};
  float o[1];
  wave_dots<1, 2>(w, v, 2 * DA, o);
  if ((threadIdx.x & 63) == 0) g.xin[j] = o[0] + g.bi[j];
}

// ---- 6, 7. residual LSTMCell ----------------------------------------------------------------------------------------
template <int KC>
__global__ __launch_bounds__(256) void ft_taco_gen_lstm_kernel(GenArgs g, int s, int layer) {
  const int L = g.L;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= L) return;
  const float *wih = layer ? g.l2ih : g.l1ih, *whh = layer ? g.l2hh : g.l1hh;
  const float *bih = layer ? g.l2bih : g.l1bih, *bhh = layer ? g.l2bhh : g.l1bhh;
  const float* x = layer ? g.x1 : g.xin;
  float* xo = layer ? g.x2 : g.x1;
  float* hb = layer ? g.h2 : g.h1;
  float* cb = layer ? g.c2 : g.c1;
  const float* hp = hb + (long)(s & 1) * L;
  const float* w[8];
  const float* v[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    w[q] = wih + (long)(q * L + j) * L; v[q] = x;
    w[4 + q] = whh + (long)(q * L + j) * L; v[4 + q] = hp;
  }
  // cell operands, requested with the dot-product operands
  float bi_[4], bh_[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { bi_[q] = bih[q * L + j]; bh_[q] = bhh[q * L + j]; }
  const float cprev = cb[(long)(s & 1) * L + j], xj = x[j];
  float o[8];
  wave_dots<8, KC>(w, v, L, o);
  if ((threadIdx.x & 63) == 0) {
    float gt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) gt[q] = ((o[q] + bi_[q]) + o[4 + q]) + bh_[q];
    const float c = ft_sigmoid(gt[1]) * cprev + ft_sigmoid(gt[0]) * ft_tanh(gt[2]);
    const float h = ft_sigmoid(gt[3]) * ft_tanh(c);
    hb[(long)((s + 1) & 1) * L + j] = h;
    cb[(long)((s + 1) & 1) * L + j] = c;
    xo[j] = xj + h;
  }
}

// ---- 8. mel_proj + stop test ----------------------------------------------------------------------------------------
template <int KC>
__global__ __launch_bounds__(256) void ft_taco_gen_mel_kernel(GenArgs g, int s) {
  __shared__ int above[4];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int i = blockIdx.x * 4 + wave;             // output row: frame k = i / 80, channel n = i % 80
  int notbelow = 0;
  if (i < GNM * g.r) {
    const int k = i / GNM, n = i - k * GNM;
    const float* w[1] = {g.wmel + (long)(n * GMAXR + k) * g.L};
    const float* v[1] = {g.x2};
    float o[1];
    wave_dots<1, KC>(w, v, g.L, o);
    if ((tid & 63) == 0) g.frames[((long)s * g.r + k) * GNM + n] = o[0];
    notbelow = !(o[0] < g.thr);                    // NaN is never below
  }
  if ((tid & 63) == 0) above[wave] = notbelow;
  __syncthreads();
  if (tid == 0) {
    if (above[0] | above[1] | above[2] | above[3]) atomicOr(g.flag, 1u);
    __threadfence();
    if (atomicAdd(g.ticket, 1u) == gridDim.x - 1) {          // last workgroup of the step
      const unsigned nb = atomicOr(g.flag, 0u);
      if (!nb && (long)s * g.r > 10 && *g.sout > s) *g.sout = s + 1;
      atomicExch(g.flag, 0u);
      atomicExch(g.ticket, 0u);
    }
  }
}

struct GenWs {
  WsLayout at;
  size_t xin, x1, x2, h1, c1, h2, c2, flag, total;
};
GenWs gen_layout(int Tx, int L) {
  GenWs w;
  w.at = ws_layout(1, Tx);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t v = sizeof(float) * (size_t)L;
  size_t o = w.at.total;
  w.xin = o; o = al(o + v);
  w.x1 = o;  o = al(o + v);
  w.x2 = o;  o = al(o + v);
  w.h1 = o;  o = al(o + 2 * v);
  w.c1 = o;  o = al(o + 2 * v);
  w.h2 = o;  o = al(o + 2 * v);
  w.c2 = o;  o = al(o + 2 * v);
  w.flag = o; o = al(o + 2 * sizeof(unsigned));
  w.total = o;
  return w;
}

}  // namespace

extern "C" {

size_t ft_taco_gen_workspace(int Tx, int lstm_dims, int r) {
  if (Tx < 1 || Tx > TXMAX || lstm_dims < 1 || r < 1 || r > GMAXR) return 0;
  return gen_layout(Tx, lstm_dims).total;
}

int ft_taco_gen_steps(const float* enc_proj, const float* enc_pq, const float* fc1_w, const float* fc1_b,
                      const float* fc2_w, const float* fc2_b, const float* w_ih, long ld_w_ih, const float* b_ih,
                      const float* w_hh, const float* b_hh, const float* W, const float* b_W, const float* conv_w,
                      const float* L, const float* b_L, const float* v, const float* rnn_in_w, const float* rnn_in_b,
                      const float* r1_w_ih, const float* r1_w_hh, const float* r1_b_ih, const float* r1_b_hh,
                      const float* r2_w_ih, const float* r2_w_hh, const float* r2_b_ih, const float* r2_b_hh,
                      const float* mel_w, float stop_threshold, float* P, float* hist, float* attn, float* frames,
                      int* s_out, int Tx, int lstm_dims, int r, int S, int s0, int n, void* ws, size_t ws_bytes,
                      void* stream) {
  FT_REQUIRE(Tx >= 1 && Tx <= TXMAX, "taco_gen_steps: Tx must be in 1..%d (got %d)", TXMAX, Tx);
  FT_REQUIRE(lstm_dims >= 1, "taco_gen_steps: lstm_dims must be >= 1 (got %d)", lstm_dims);
  FT_REQUIRE(r >= 1 && r <= GMAXR, "taco_gen_steps: r must be in 1..%d (got %d)", GMAXR, r);
  FT_REQUIRE(S >= 1 && s0 >= 0 && n >= 0 && (long)s0 + n <= S,
             "taco_gen_steps: steps [%d, %d) must lie in [0, S = %d)", s0, s0 + n, S);
  FT_REQUIRE(ld_w_ih >= DA + GF2 && ld_w_ih % 4 == 0, "taco_gen_steps: ld_w_ih must be a multiple of 4, >= 384");
  FT_REQUIRE(enc_proj && enc_pq && fc1_w && fc1_b && fc2_w && fc2_b && w_ih && b_ih && w_hh && b_hh && W && b_W &&
             conv_w && L && b_L && v && rnn_in_w && rnn_in_b && r1_w_ih && r1_w_hh && r1_b_ih && r1_b_hh && r2_w_ih &&
             r2_w_hh && r2_b_ih && r2_b_hh && mel_w && P && hist && attn && frames && s_out,
             "taco_gen_steps: null operand");
  const bool v4 = lstm_dims % 4 == 0;
  FT_REQUIRE(al16(fc1_w) && al16(fc2_w) && al16(w_ih) && al16(w_hh) && al16(W) && al16(L) && al16(rnn_in_w) &&
             al16(hist) && al16(ws) && (!v4 || (al16(r1_w_ih) && al16(r1_w_hh) && al16(r2_w_ih) && al16(r2_w_hh) &&
                                                al16(mel_w))),
             "taco_gen_steps: weights, history and workspace must be 16-byte aligned");
  const GenWs wl = gen_layout(Tx, lstm_dims);
  FT_REQUIRE(ws && ws_bytes >= wl.total, "taco_gen_steps: workspace too small (%zu < %zu bytes)", ws_bytes, wl.total);
  if (n == 0) return FT_OK;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  AttendArgs a;
  a.enc_proj = enc_proj; a.enc_pq = enc_pq; a.P = P; a.wih = w_ih; a.ld_wih = ld_w_ih; a.whh = w_hh; a.bhh = b_hh;
  a.W = W; a.bW = b_W; a.cw = conv_w; a.L = L; a.bL = b_L; a.v = v; a.attn = attn;
  a.qp = (float*)(w + wl.at.qp); a.E = (float*)(w + wl.at.E); a.cum = (float*)(w + wl.at.cum);
  a.att = (float*)(w + wl.at.att);
  a.B = 1; a.Tx = Tx; a.S = S;
  a.ldh = 2 * DA; a.lens = nullptr;
  GenArgs g;
  g.fc1w = fc1_w; g.fc1b = fc1_b; g.fc2w = fc2_w; g.fc2b = fc2_b; g.wih = w_ih; g.ld_wih = ld_w_ih; g.bih = b_ih;
  g.wi = rnn_in_w; g.bi = rnn_in_b;
  g.l1ih = r1_w_ih; g.l1hh = r1_w_hh; g.l1bih = r1_b_ih; g.l1bhh = r1_b_hh;
  g.l2ih = r2_w_ih; g.l2hh = r2_w_hh; g.l2bih = r2_b_ih; g.l2bhh = r2_b_hh;
  g.wmel = mel_w; g.thr = stop_threshold;
  g.P = P; g.hist = hist; g.frames = frames; g.sout = s_out;
  g.xin = (float*)(w + wl.xin); g.x1 = (float*)(w + wl.x1); g.x2 = (float*)(w + wl.x2);
  g.h1 = (float*)(w + wl.h1); g.c1 = (float*)(w + wl.c1); g.h2 = (float*)(w + wl.h2); g.c2 = (float*)(w + wl.c2);
  g.flag = (unsigned*)(w + wl.flag); g.ticket = g.flag + 1;
  g.L = lstm_dims; g.r = r; g.S = S;
  // s0 == 0: LSA state, LSTM states, stop flag and ticket from zero (S_out := S by the first prenet launch); the GRU
  // kernel takes h = context = 0 at s = 0 itself
  if (s0 == 0) (void)hipMemsetAsync(w + wl.at.cum, 0, wl.total - wl.at.cum, st);
  const dim3 g1(NUB, 1), g2(ft_cdiv(Tx, TC), 1, NCQ), g3(NAC, 1);
  const dim3 gl(ft_cdiv(lstm_dims, 4)), gm(ft_cdiv(GNM * r, 4));
  const bool fast = lstm_dims == 512;
  for (int s = s0; s < s0 + n; ++s) {
    const float* prev = hist + (long)(s > 0 ? s - 1 : 0) * 2 * DA;
    float* cur = hist + (long)s * 2 * DA;
    hipLaunchKernelGGL(ft_taco_gen_prenet_kernel, dim3(GPB), dim3(1024), 0, st, g, s);
    hipLaunchKernelGGL(ft_taco_gru_kernel, g1, dim3(256), 0, st, a, s, prev + DA, prev, cur + DA);
    hipLaunchKernelGGL(ft_taco_energy_kernel, g2, dim3(256), 0, st, a);
    hipLaunchKernelGGL(ft_taco_context_kernel, g3, dim3(256), 0, st, a, s, cur);
    hipLaunchKernelGGL(ft_taco_gen_rnnin_kernel, gl, dim3(256), 0, st, g, s);
    if (fast) {
      hipLaunchKernelGGL(ft_taco_gen_lstm_kernel<2>, gl, dim3(256), 0, st, g, s, 0);
      hipLaunchKernelGGL(ft_taco_gen_lstm_kernel<2>, gl, dim3(256), 0, st, g, s, 1);
      hipLaunchKernelGGL(ft_taco_gen_mel_kernel<2>, gm, dim3(256), 0, st, g, s);
    } else {
      hipLaunchKernelGGL(ft_taco_gen_lstm_kernel<0>, gl, dim3(256), 0, st, g, s, 0);
      hipLaunchKernelGGL(ft_taco_gen_lstm_kernel<0>, gl, dim3(256), 0, st, g, s, 1);
      hipLaunchKernelGGL(ft_taco_gen_mel_kernel<0>, gm, dim3(256), 0, st, g, s);
    }
  }
  return ft_check_launch("taco_gen_steps");
}

}  // extern "C"

// =====================================================================================================================
// Autoregressive generate of a RAGGED BATCH (Tacotron.generate_batch): B sentences, item b with lens[b] <= Tx tokens.
//
// Masking rule (what makes item b equal the sentence run alone at Tx = lens[b]): energies are formed and the softmax
// runs over t < lens[b] only; attention and cumulative stay exact zeros at t >= lens[b], so the location conv sees at
// the item's end the zero padding it sees at a sequence end; the context sums t < lens[b]; no row of enc_proj / enc_pq
// past an item's length is loaded.  ft_taco_energy_kernel and ft_taco_context_kernel take that from AttendArgs.lens.
//
// A step is eight launches, as at B = 1, but a tile of 16 items shares every weight read: each decoder cell is a
// skinny product [16 items x K] x [K x 16 columns] on v_mfma_f32_16x16x4_f32 with K split over the four waves of the
// workgroup (the shape of ft_taco_gru_kernel), a fixed-order sum of the four partial tiles through LDS, then the cell
// epilogue.  Grid = (column blocks, ceil(B / 16) item tiles):
//   1. ft_taco_bgen_prenet_kernel  (12, tiles): the 16 last frames -> fc1 + ReLU -> fc2 + ReLU in LDS (recomputed by
//        each of the 12 workgroups, as at B = 1: L2 reads instead of two launches), then 64 of P[s]'s 768 columns.
//        Here the waves split the COLUMNS (16 per wave and tile), each wave sums its whole K in ascending order.
//   2-4. ft_taco_gru_kernel, ft_taco_energy_kernel, ft_taco_context_kernel with lens.
//   5. ft_taco_bgen_rnnin_kernel   (ceil(L/16), tiles): K = 512, 128 per wave.
//   6, 7. ft_taco_bgen_lstm_kernel (ceil(L/4), tiles): 16 columns = 4 units x gates (i, f, g, o); waves 0, 1 take x
//        against W_ih, waves 2, 3 take h against W_hh; h and c ping-pong on the parity of s; x + h' is the output.
//   8. ft_taco_bgen_mel_kernel     (ceil(80 r / 16), tiles): rows n*20 + k, k < r -> frames[b][s*r + k][n]; one "not
//        below" flag word per item, ORed by the workgroups that hold a value of the item that is not below the
//        threshold; the last workgroup of the launch (ticket counter; the atomics count and flag, they never carry
//        values) sets s_out[b] = s + 1 the first time item b's test holds.
// An item that has stopped keeps being stepped (its later slots are masked by the caller); no kernel sums across
// items, so this cannot touch another item.  lstm_dims = 512 takes the template path whose loads all precede the
// first dependent MFMA; any other width takes a loop in 16-wide K chunks (float4 loads when lstm_dims % 4 == 0).
// Rows of a partly filled tile read the last item and columns past the end read the last row; neither is stored.
namespace {

struct BGenArgs {
  GenArgs g;      // P [S,B,768], hist [S,B,512], frames [B,S*r,80], sout [B]; xin, x1, x2 [B,L]; h*, c* [2][B,L];
  int B;          // flag [B] words, ticket one word
};

// One wave's share of a [16 x K] x [K x 16] product: arow / brow are the lane's operand rows (item l15, column l15),
// the wave sums k in [k0, k1) in ascending 16-wide chunks.  KC > 0: k1 - k0 == 16 KC and the rows are 16-byte
// aligned, every load is issued before the first MFMA.  vec: float4 loads (rows aligned, k1 - k0 a multiple of 4).
template <int KC>
__device__ __forceinline__ f32x4 skinny16(const float* arow, const float* brow, int k0, int k1, bool vec) {
  const int q = (threadIdx.x & 63) >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if constexpr (KC > 0) {
    float4 av[KC], bv[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      av[c] = ld4(arow + k0 + 16 * c + 4 * q);
      bv[c] = ld4(brow + k0 + 16 * c + 4 * q);
    }
    __builtin_amdgcn_sched_barrier(0);      // keep the scheduler from sinking loads between the MFMAs
#pragma unroll
    for (int c = 0; c < KC; ++c) mfma4(av[c], bv[c], acc);
  } else {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kb = k0; kb < k1; kb += 16) {            // wave-uniform trip count: every lane issues every MFMA
      const int k = kb + 4 * q;
      float4 a = z, b = z;
      if (vec) {
        if (k < k1) { a = ld4(arow + k); b = ld4(brow + k); }
      } else {
        if (k < k1) { a.x = arow[k]; b.x = brow[k]; }
        if (k + 1 < k1) { a.y = arow[k + 1]; b.y = brow[k + 1]; }
        if (k + 2 < k1) { a.z = arow[k + 2]; b.z = brow[k + 2]; }
        if (k + 3 < k1) { a.w = arow[k + 3]; b.w = brow[k + 3]; }
      }
      mfma4(a, b, acc);
    }
  }
  return acc;
}

// the K range of wave `w` of `nw` waves that share K in 16-wide chunks
__device__ __forceinline__ void k_slice(int K, int w, int nw, int& k0, int& k1) {
  const int cpw = ((K + 15) / 16 + nw - 1) / nw * 16;
  k0 = min(K, w * cpw);
  k1 = min(K, k0 + cpw);
}

__device__ __forceinline__ void store_tile(float (&red)[4][16][17], const f32x4& acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, q = lane >> 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) red[wave][4 * q + e][l15] = acc[e];
}

// ---- 1. decoder prenet + prenet half of the GRU input projection, 16 items ----------------------------------------
constexpr int BPB = 12;          // prenet workgroups per item tile: 64 columns of P each, 16 per wave
__global__ __launch_bounds__(256) void ft_taco_bgen_prenet_kernel(BGenArgs ba, int s) {
  constexpr int LF = GNM + 4, L1 = GF1 + 4, L2 = GF2 + 4;       // LDS row strides: 16-byte aligned rows
  constexpr int C1 = GNM / 16, C2 = GF1 / 16, C3 = GF2 / 16;    // K chunks
  static_assert(GNM % 16 == 0 && NG == BPB * 64, "prenet shape");
  __shared__ __attribute__((aligned(16))) float f[16][LF];
  __shared__ __attribute__((aligned(16))) float p1[16][L1];
  __shared__ __attribute__((aligned(16))) float p2[16][L2];
  const GenArgs& g = ba.g;
  const int B = ba.B, b0 = blockIdx.y * 16;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
  if (s == 0 && blockIdx.x == 0 && tid < 16 && b0 + tid < B) g.sout[b0 + tid] = g.S;
  // every weight of the three products is requested with the frames
  float4 w1[4][C1], w2[2][C2], w3[C3];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int c = 0; c < C1; ++c) w1[t][c] = ld4(g.fc1w + (long)(64 * wave + 16 * t + l15) * GNM + 16 * c + 4 * q);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < C2; ++c) w2[t][c] = ld4(g.fc2w + (long)(32 * wave + 16 * t + l15) * GF1 + 16 * c + 4 * q);
  const int col3 = 64 * blockIdx.x + 16 * wave + l15;
#pragma unroll
  for (int c = 0; c < C3; ++c) w3[c] = ld4(g.wih + (long)col3 * g.ld_wih + DA + 16 * c + 4 * q);
  float b1[4], b2[2];
#pragma unroll
  for (int t = 0; t < 4; ++t) b1[t] = g.fc1b[64 * wave + 16 * t + l15];
#pragma unroll
  for (int t = 0; t < 2; ++t) b2[t] = g.fc2b[32 * wave + 16 * t + l15];
  const float b3 = g.bih[col3];
  for (int i = tid; i < 16 * GNM; i += 256) {
    const int it = i / GNM, ch = i - it * GNM, b = b0 + it;
    f[it][ch] = (s > 0 && b < B) ? g.frames[((long)b * g.S * g.r + (long)s * g.r - 1) * GNM + ch] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < C1; ++c) mfma4(ld4(&f[l15][16 * c + 4 * q]), w1[t][c], acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) p1[4 * q + e][64 * wave + 16 * t + l15] = fmaxf(acc[e] + b1[t], 0.f);
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < C2; ++c) mfma4(ld4(&p1[l15][16 * c + 4 * q]), w2[t][c], acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) p2[4 * q + e][32 * wave + 16 * t + l15] = fmaxf(acc[e] + b2[t], 0.f);
  }
  __syncthreads();
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < C3; ++c) mfma4(ld4(&p2[l15][16 * c + 4 * q]), w3[c], acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = b0 + 4 * q + e;
      if (b < B) g.P[((long)s * B + b) * NG + col3] = acc[e] + b3;
    }
  }
}

// ---- 5. rnn_input, 16 items x 16 outputs ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ft_taco_bgen_rnnin_kernel(BGenArgs ba, int s) {
  __shared__ float red[4][16][17];
  const GenArgs& g = ba.g;
  const int B = ba.B, L = g.L, b0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  const int tid = threadIdx.x, wave = tid >> 6, l15 = tid & 15;
  const int it = tid >> 4, cb = b0 + it, cj = j0 + l15;
  const bool act = cb < B && cj < L;
  const float bias = act ? g.bi[cj] : 0.f;
  const float* arow = g.hist + ((long)s * B + min(b0 + l15, B - 1)) * 2 * DA;
  const float* brow = g.wi + (long)min(j0 + l15, L - 1) * 2 * DA;
  constexpr int KW4 = 2 * DA / 4;                 // K per wave
  store_tile(red, skinny16<KW4 / 16>(arow, brow, KW4 * wave, KW4 * (wave + 1), true));
  __syncthreads();
  if (act) g.xin[(long)cb * L + cj] = ((red[0][it][l15] + red[1][it][l15]) + (red[2][it][l15] + red[3][it][l15])) + bias;
}

// ---- 6, 7. residual LSTMCell, 16 items x 4 units ------------------------------------------------------------------------
template <int KC>
__global__ __launch_bounds__(256) void ft_taco_bgen_lstm_kernel(BGenArgs ba, int s, int layer) {
  __shared__ float red[4][16][17];
  const GenArgs& g = ba.g;
  const int B = ba.B, L = g.L, b0 = blockIdx.y * 16, u0 = blockIdx.x * 4;
  const int tid = threadIdx.x, wave = tid >> 6, l15 = tid & 15;
  const float *wih = layer ? g.l2ih : g.l1ih, *whh = layer ? g.l2hh : g.l1hh;
  const float *bih = layer ? g.l2bih : g.l1bih, *bhh = layer ? g.l2bhh : g.l1bhh;
  const float* x = layer ? g.x1 : g.xin;
  float* xo = layer ? g.x2 : g.x1;
  float* hb = layer ? g.h2 : g.h1;
  float* cbuf = layer ? g.c2 : g.c1;
  const long par = (long)(s & 1) * B * L, nxt = (long)((s + 1) & 1) * B * L;
  // cell operands of thread tid < 64 (item tid / 4, unit u0 + tid % 4), requested with the product's operands
  const int it = tid >> 2, cb = b0 + it, cu = u0 + (tid & 3);
  const bool act = tid < 64 && cb < B && cu < L;
  float bi_[4] = {0.f, 0.f, 0.f, 0.f}, bh_[4] = {0.f, 0.f, 0.f, 0.f}, cprev = 0.f, xj = 0.f;
  if (act) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { bi_[q] = bih[q * L + cu]; bh_[q] = bhh[q * L + cu]; }
    cprev = cbuf[par + (long)cb * L + cu];
    xj = x[(long)cb * L + cu];
  }
  const int seg = wave >> 1;                         // 0: x against W_ih, 1: h against W_hh
  const long bA = min(b0 + l15, B - 1);
  const float* arow = (seg ? hb + par : x) + bA * L;
  const float* brow = (seg ? whh : wih) + ((long)(l15 & 3) * L + min(u0 + (l15 >> 2), L - 1)) * L;
  int k0, k1;
  if constexpr (KC > 0) { k0 = 16 * KC * (wave & 1); k1 = k0 + 16 * KC; } else { k_slice(L, wave & 1, 2, k0, k1); }
  store_tile(red, skinny16<KC>(arow, brow, k0, k1, (L & 3) == 0));
  __syncthreads();
  if (act) {
    const int c0 = 4 * (tid & 3);
    float gt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      gt[q] = (((red[0][it][c0 + q] + red[1][it][c0 + q]) + bi_[q]) + (red[2][it][c0 + q] + red[3][it][c0 + q])) + bh_[q];
    const float c = ft_sigmoid(gt[1]) * cprev + ft_sigmoid(gt[0]) * ft_tanh(gt[2]);
    const float h = ft_sigmoid(gt[3]) * ft_tanh(c);
    hb[nxt + (long)cb * L + cu] = h;
    cbuf[nxt + (long)cb * L + cu] = c;
    xo[(long)cb * L + cu] = xj + h;
  }
}

// ---- 8. mel_proj + per-item stop test ---------------------------------------------------------------------------------
template <int KC>
__global__ __launch_bounds__(256) void ft_taco_bgen_mel_kernel(BGenArgs ba, int s) {
  __shared__ float red[4][16][17];
  __shared__ int last;
  const GenArgs& g = ba.g;
  const int B = ba.B, L = g.L, b0 = blockIdx.y * 16, i0 = blockIdx.x * 16, rows = GNM * g.r;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = tid & 15;
  const int ib = min(i0 + l15, rows - 1);            // output row of the lane's weight row: frame k, channel n
  const float* arow = g.x2 + (long)min(b0 + l15, B - 1) * L;
  const float* brow = g.wmel + (long)((ib % GNM) * GMAXR + ib / GNM) * L;
  int k0, k1;
  if constexpr (KC > 0) { k0 = 16 * KC * wave; k1 = k0 + 16 * KC; } else { k_slice(L, wave, 4, k0, k1); }
  store_tile(red, skinny16<KC>(arow, brow, k0, k1, (L & 3) == 0));
  __syncthreads();
  const int it = tid >> 4, cb = b0 + it, i = i0 + l15;
  int notbelow = 0;
  if (cb < B && i < rows) {
    const float v = (red[0][it][l15] + red[1][it][l15]) + (red[2][it][l15] + red[3][it][l15]);
    const int k = i / GNM, n = i - k * GNM;
    g.frames[((long)cb * g.S * g.r + (long)s * g.r + k) * GNM + n] = v;
    notbelow = !(v < g.thr);                         // NaN is never below
  }
  // the 16 lanes that share lane >> 4 hold one item
  const unsigned long long m = __ballot(notbelow);
  if (l15 == 0 && ((m >> (lane & 48)) & 0xFFFFull)) atomicOr(g.flag + cb, 1u);
  __threadfence();
  __syncthreads();
  if (tid == 0) last = atomicAdd(g.ticket, 1u) == gridDim.x * gridDim.y - 1;
  __syncthreads();
  if (last) {                                        // last workgroup of the step: one decision per item
    __threadfence();
    for (int b = tid; b < B; b += 256) {
      const unsigned nb = atomicOr(g.flag + b, 0u);
      if (!nb && (long)s * g.r > 10 && g.sout[b] > s) g.sout[b] = s + 1;
      atomicExch(g.flag + b, 0u);
    }
    if (tid == 0) atomicExch(g.ticket, 0u);
  }
}

struct BGenWs {
  WsLayout at;
  size_t xin, x1, x2, h1, c1, h2, c2, flag, total;
};
BGenWs bgen_layout(int B, int Tx, int L) {
  BGenWs w;
  w.at = ws_layout(B, Tx);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t v = sizeof(float) * (size_t)B * L;
  size_t o = w.at.total;
  w.xin = o; o = al(o + v);
  w.x1 = o;  o = al(o + v);
  w.x2 = o;  o = al(o + v);
  w.h1 = o;  o = al(o + 2 * v);
  w.c1 = o;  o = al(o + 2 * v);
  w.h2 = o;  o = al(o + 2 * v);
  w.c2 = o;  o = al(o + 2 * v);
  w.flag = o; o = al(o + ((size_t)B + 1) * sizeof(unsigned));
  w.total = o;
  return w;
}

constexpr int BGEN_MAXB = 65535;     // the energy and context grids carry the item in gridDim.y

}  // namespace

extern "C" {

size_t ft_taco_gen_batch_workspace(int B, int Tx, int lstm_dims, int r) {
  if (B < 1 || B > BGEN_MAXB || Tx < 1 || Tx > TXMAX || lstm_dims < 1 || r < 1 || r > GMAXR) return 0;
  return bgen_layout(B, Tx, lstm_dims).total;
}

int ft_taco_gen_batch_steps(const float* enc_proj, const float* enc_pq, const float* fc1_w, const float* fc1_b,
                            const float* fc2_w, const float* fc2_b, const float* w_ih, long ld_w_ih, const float* b_ih,
                            const float* w_hh, const float* b_hh, const float* W, const float* b_W,
                            const float* conv_w, const float* L, const float* b_L, const float* v,
                            const float* rnn_in_w, const float* rnn_in_b, const float* r1_w_ih, const float* r1_w_hh,
                            const float* r1_b_ih, const float* r1_b_hh, const float* r2_w_ih, const float* r2_w_hh,
                            const float* r2_b_ih, const float* r2_b_hh, const float* mel_w, float stop_threshold,
                            float* P, float* hist, float* attn, float* frames, int* s_out, const long* lens, int B,
                            int Tx, int lstm_dims, int r, int S, int s0, int n, void* ws, size_t ws_bytes,
                            void* stream) {
  FT_REQUIRE(B >= 1 && B <= BGEN_MAXB, "taco_gen_batch_steps: B must be in 1..%d (got %d)", BGEN_MAXB, B);
  FT_REQUIRE(Tx >= 1 && Tx <= TXMAX, "taco_gen_batch_steps: Tx must be in 1..%d (got %d)", TXMAX, Tx);
  FT_REQUIRE(lstm_dims >= 1, "taco_gen_batch_steps: lstm_dims must be >= 1 (got %d)", lstm_dims);
  FT_REQUIRE(r >= 1 && r <= GMAXR, "taco_gen_batch_steps: r must be in 1..%d (got %d)", GMAXR, r);
  FT_REQUIRE(S >= 1 && s0 >= 0 && n >= 0 && (long)s0 + n <= S,
             "taco_gen_batch_steps: steps [%d, %d) must lie in [0, S = %d)", s0, s0 + n, S);
  FT_REQUIRE(ld_w_ih >= DA + GF2 && ld_w_ih % 4 == 0,
             "taco_gen_batch_steps: ld_w_ih must be a multiple of 4, >= 384");
  FT_REQUIRE(enc_proj && enc_pq && fc1_w && fc1_b && fc2_w && fc2_b && w_ih && b_ih && w_hh && b_hh && W && b_W &&
             conv_w && L && b_L && v && rnn_in_w && rnn_in_b && r1_w_ih && r1_w_hh && r1_b_ih && r1_b_hh && r2_w_ih &&
             r2_w_hh && r2_b_ih && r2_b_hh && mel_w && P && hist && attn && frames && s_out && lens,
             "taco_gen_batch_steps: null operand");
  const bool v4 = lstm_dims % 4 == 0;
  FT_REQUIRE(al16(fc1_w) && al16(fc2_w) && al16(w_ih) && al16(w_hh) && al16(W) && al16(L) && al16(rnn_in_w) &&
             al16(hist) && al16(ws) && (!v4 || (al16(r1_w_ih) && al16(r1_w_hh) && al16(r2_w_ih) && al16(r2_w_hh) &&
                                                al16(mel_w))),
             "taco_gen_batch_steps: weights, history and workspace must be 16-byte aligned");
  const BGenWs wl = bgen_layout(B, Tx, lstm_dims);
  FT_REQUIRE(ws && ws_bytes >= wl.total, "taco_gen_batch_steps: workspace too small (%zu < %zu bytes)", ws_bytes,
             wl.total);
  if (n == 0) return FT_OK;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  AttendArgs a;
  a.enc_proj = enc_proj; a.enc_pq = enc_pq; a.P = P; a.wih = w_ih; a.ld_wih = ld_w_ih; a.whh = w_hh; a.bhh = b_hh;
  a.W = W; a.bW = b_W; a.cw = conv_w; a.L = L; a.bL = b_L; a.v = v; a.attn = attn;
  a.qp = (float*)(w + wl.at.qp); a.E = (float*)(w + wl.at.E); a.cum = (float*)(w + wl.at.cum);
  a.att = (float*)(w + wl.at.att);
  a.B = B; a.Tx = Tx; a.S = S;
  a.ldh = 2 * DA; a.lens = lens;
  BGenArgs ba;
  GenArgs& g = ba.g;
  g.fc1w = fc1_w; g.fc1b = fc1_b; g.fc2w = fc2_w; g.fc2b = fc2_b; g.wih = w_ih; g.ld_wih = ld_w_ih; g.bih = b_ih;
  g.wi = rnn_in_w; g.bi = rnn_in_b;
  g.l1ih = r1_w_ih; g.l1hh = r1_w_hh; g.l1bih = r1_b_ih; g.l1bhh = r1_b_hh;
  g.l2ih = r2_w_ih; g.l2hh = r2_w_hh; g.l2bih = r2_b_ih; g.l2bhh = r2_b_hh;
  g.wmel = mel_w; g.thr = stop_threshold;
  g.P = P; g.hist = hist; g.frames = frames; g.sout = s_out;
  g.xin = (float*)(w + wl.xin); g.x1 = (float*)(w + wl.x1); g.x2 = (float*)(w + wl.x2);
  g.h1 = (float*)(w + wl.h1); g.c1 = (float*)(w + wl.c1); g.h2 = (float*)(w + wl.h2); g.c2 = (float*)(w + wl.c2);
  g.flag = (unsigned*)(w + wl.flag); g.ticket = g.flag + B;
  g.L = lstm_dims; g.r = r; g.S = S;
  ba.B = B;
  // s0 == 0: LSA state, LSTM states, stop flags and ticket from zero (s_out[b] := S by the first prenet launch)
  if (s0 == 0) (void)hipMemsetAsync(w + wl.at.cum, 0, wl.total - wl.at.cum, st);
  const unsigned tiles = ft_cdiv(B, 16);
  const dim3 g1(NUB, tiles), g2(ft_cdiv(Tx, TC), B, NCQ), g3(NAC, B);
  const dim3 gp(BPB, tiles), gi(ft_cdiv(lstm_dims, 16), tiles), gl(ft_cdiv(lstm_dims, 4), tiles);
  const dim3 gm(ft_cdiv(GNM * r, 16), tiles);
  const bool fast = lstm_dims == 512;
  const long slab = (long)B * 2 * DA;
  for (int s = s0; s < s0 + n; ++s) {
    const float* prev = hist + (long)(s > 0 ? s - 1 : 0) * slab;
    float* cur = hist + (long)s * slab;
    hipLaunchKernelGGL(ft_taco_bgen_prenet_kernel, gp, dim3(256), 0, st, ba, s);
    hipLaunchKernelGGL(ft_taco_gru_kernel, g1, dim3(256), 0, st, a, s, prev + DA, prev, cur + DA);
    hipLaunchKernelGGL(ft_taco_energy_kernel, g2, dim3(256), 0, st, a);
    hipLaunchKernelGGL(ft_taco_context_kernel, g3, dim3(256), 0, st, a, s, cur);
    hipLaunchKernelGGL(ft_taco_bgen_rnnin_kernel, gi, dim3(256), 0, st, ba, s);
    if (fast) {
      hipLaunchKernelGGL(ft_taco_bgen_lstm_kernel<16>, gl, dim3(256), 0, st, ba, s, 0);
      hipLaunchKernelGGL(ft_taco_bgen_lstm_kernel<16>, gl, dim3(256), 0, st, ba, s, 1);
      hipLaunchKernelGGL(ft_taco_bgen_mel_kernel<8>, gm, dim3(256), 0, st, ba, s);
    } else {
      hipLaunchKernelGGL(ft_taco_bgen_lstm_kernel<0>, gl, dim3(256), 0, st, ba, s, 0);
      hipLaunchKernelGGL(ft_taco_bgen_lstm_kernel<0>, gl, dim3(256), 0, st, ba, s, 1);
      hipLaunchKernelGGL(ft_taco_bgen_mel_kernel<0>, gm, dim3(256), 0, st, ba, s);
    }
  }
  return ft_check_launch("taco_gen_batch_steps");
}

}  // extern "C"
