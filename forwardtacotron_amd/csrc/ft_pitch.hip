// Raw pitch of a ragged batch of wavs: probabilistic YIN (Mauch & Dixon 2014) with librosa.pyin's documented defaults
// (reference: pitch_extraction/pitch_extractor.py:24-47 LibrosaPitchExtractor, called from preprocess.py:90 right after
// wav_to_mel).  Three launches; the definition each implements is in include/fwdtaco_hip.h and DESIGN.md section 7, the
// numpy restatement in tests/pyin_cpu.py.
//   ft_pyin_cmnd     wav -> cumulative-mean-normalised difference function dn [B, Tmax, P], fp32, the squared
//                    differences formed directly (no energy - 2 acf expansion, which cancels)
//   ft_pyin_observe  dn -> log observation probabilities of the 2N-state HMM: lo_v [B, Tmax, N], lo_u, vp [B, Tmax]
//   ft_pyin_viterbi  lo_v, lo_u -> state path, score and pitch; one workgroup per item, T_b dependent steps
// Every kernel reads the per-item lengths on the device, clamps them, writes defined values past an item's frames, and
// loads nothing past a length: NaN in the padding or in a neighbour reaches nothing.  Every loop is bounded by host
// values, so a NaN item finishes.  No atomics on values (one LDS integer max decides which candidate owns a pitch bin),
// no cross-workgroup waits.  The probability sums and the Viterbi recursion are single fp32 operations in a stated order
// (no contraction: the pragma below), so tests/pyin_cpu.py reproduces them bit for bit.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "ft_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kFrames = 4;                  // cmnd: frames per workgroup = waves per workgroup
constexpr int kCmndThreads = 256;
constexpr int kObsThreads = 512;            // observe: one trough slot per thread
constexpr int kMaxP = 1024;                 // observe: periods per frame; troughs are never adjacent, so at most 512
constexpr int kThr = 100;                   // thresholds
constexpr int kVitThreads = 1024;
constexpr int kMaxN = 1024;                 // viterbi: 2N <= 2048 states, at most two per thread
constexpr int kMaxHalf = 2048;
constexpr size_t kLdsBudget = 65536;


// ---------------------------------------------------------------------------------------------------------------------
// stage 1.  A workgroup owns kFrames consecutive frames of one item and stages their samples once (consecutive frames
// share frame_length - hop samples).  A task is (frame, four consecutive lags): for each j the thread holds x_j in a
// register and a sliding window x[j + tau0 .. j + tau0 + 6], 16 subtract + fma pairs for 8 LDS words.  d(tau) is one
// sequential fma chain over j = 0 .. W - 1 whatever the batch.  Then one wave per frame forms the prefix sums (each lane a
// run of consecutive lags, a shuffle scan over the runs) and dn.
// LDS: xs [frame_length + (kFrames - 1) hop + 8] | d [kFrames][DP], DP = (pmax + 4) & ~3.
struct CmndGeom { int span, DP; };
__host__ __device__ inline CmndGeom py_cmnd_geom(int fl, int hop, int pmax) {
  CmndGeom g;
  g.span = (fl + (kFrames - 1) * hop + 8 + 3) & ~3;
  g.DP = (pmax + 4) & ~3;
  return g;
}

template <bool VEC>
__global__ __launch_bounds__(kCmndThreads) void py_cmnd_kernel(const float* __restrict__ x, long ldx,
                                                               const long* __restrict__ len, long Lmax, int fl, int hop,
                                                               int pmin, int pmax, int Tmax, float* __restrict__ dn,
                                                               long* __restrict__ frames) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long L = ft_item_len(len, b, 0, Lmax, nullptr);
  const int T = (int)(1 + L / hop);                                     // <= Tmax = 1 + Lmax / hop
  if (blockIdx.x == 0 && tid == 0) frames[b] = T;
  const int t0 = blockIdx.x * kFrames;
  const int P = pmax - pmin + 1, W = fl / 2;
  const int nf = min(kFrames, Tmax - t0);                               // frames this workgroup writes
  const int nv = max(0, min(nf, T - t0));                               // of which the item has
  float* dnb = dn + ((long)b * Tmax + t0) * P;
  for (int i = nv * P + tid; i < nf * P; i += kCmndThreads) dnb[i] = 0.f;
  if (nv == 0) return;
  const CmndGeom g = py_cmnd_geom(fl, hop, pmax);
  float* xs = lds;
  float* dd = lds + g.span;
  const float* xr = x + (long)b * ldx;
  const long s0 = (long)t0 * hop - fl / 2;                              // the wav index of xs[0]: zero padding of fl / 2
  for (int i = tid; i < g.span; i += kCmndThreads) {
    const long k = s0 + i;
    xs[i] = (k >= 0 && k < L) ? xr[k] : 0.f;
  }
  __syncthreads();
  const int nblk = g.DP / 4, W4 = W & ~3;
  for (int task = tid; task < nv * nblk; task += kCmndThreads) {
    const int f = task / nblk, tau0 = 4 * (task - f * nblk);
    const float* xf = xs + f * hop;
    const float* xw = xf + tau0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float w[8];
    if (VEC) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xw);
      w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = xw[e];
    }
    for (int j0 = 0; j0 < W4; j0 += 4) {
      float a[4];
      if (VEC) {
        const f32x4 va = *reinterpret_cast<const f32x4*>(xf + j0);
        const f32x4 vw = *reinterpret_cast<const f32x4*>(xw + j0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = va[e]; w[4 + e] = vw[e]; }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = xf[j0 + e]; w[4 + e] = xw[j0 + 4 + e]; }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float df = a[c] - w[c + r];
          acc[r] = fmaf(df, df, acc[r]);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = w[4 + e];
    }
    for (int j = W4; j < W; ++j) {                                      // W % 4 samples, the same chain
      const float a = xf[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float df = a - xw[j + r];
        acc[r] = fmaf(df, df, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dd[f * g.DP + tau0 + r] = acc[r];
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int f = wave; f < nv; f += kCmndThreads / 64) {
    float* df = dd + f * g.DP;
    const int ch = (pmax + 63) / 64;                                    // lags 1 .. pmax in 64 runs of ch
    const int lo = 1 + lane * ch, hi = min(pmax, lo + ch - 1);
    float run = 0.f;
    for (int tau = lo; tau <= hi; ++tau) run += df[tau];
    float inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    const float before = __shfl_up(inc, 1, 64);                         // the runs before this lane's
    float c = lane == 0 ? 0.f : before;
    for (int tau = lo; tau <= hi; ++tau) {
      const float d = df[tau];
      c += d;
      df[tau] = d / fmaxf(c / (float)tau, FLT_MIN);
    }
  }
  __syncthreads();
  for (int i = tid; i < nv * P; i += kCmndThreads) {
    const int f = i / P, q = i - f * P;
    dnb[i] = dd[f * g.DP + pmin + q];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// stage 2.  One workgroup per frame.  Troughs are compacted in ascending period order, one per thread; per threshold k a
// wave ballot counts the troughs below it, so pos(i, k) = troughs of earlier waves + earlier lanes, n(k) = all of them.
__device__ __forceinline__ int py_block_excl_scan(int v, int* wtot, int tid, int* total) {
  const int lane = tid & 63, wave = tid >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w2 = 0; w2 < kObsThreads / 64; ++w2) {
    const int c = wtot[w2];
    base += w2 < wave ? c : 0;
    tot += c;
  }
  *total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(kObsThreads) void py_observe_kernel(
    const float* __restrict__ dn, const long* __restrict__ frames, int Tmax, int P, int pmin, int N, double sr, double fmin,
    const float* __restrict__ thr, const float* __restrict__ bp, const float* __restrict__ bpc, const float* __restrict__ E,
    const float* __restrict__ C, int nE, float LZ, float* __restrict__ lo_v, float* __restrict__ lo_u,
    float* __restrict__ vp, float* __restrict__ prob, int* __restrict__ info, short* __restrict__ posd) {
  __shared__ float h[kMaxP];
  __shared__ int tr_i[kMaxP / 2];
  __shared__ float tr_h[kMaxP / 2];
  __shared__ float tr_p[kMaxP / 2];
  __shared__ float pi[kMaxP];                                           // p_i by period, -1 where there is no trough
  __shared__ int own[kMaxN];
  __shared__ float sE[kMaxP / 2 + 1], sC[kMaxP / 2 + 1];
  __shared__ float sthr[kThr], sbp[kThr];
  __shared__ int cnt[kObsThreads / 64 + 1][kThr];                      // per wave, then exclusive over the waves | n(k)
  __shared__ int wtot[kObsThreads / 64];
  __shared__ float wminh[kObsThreads / 64];
  __shared__ int wminq[kObsThreads / 64];
  __shared__ float wsum[kObsThreads / 64];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = (int)ft_item_len(frames, b, 0, Tmax, nullptr);
  const bool live = t < T;
  const long row = (long)b * Tmax + t;
  if (!live) {                                                          // past the item: what a frame of dn = 0 gives
    for (int s = tid; s < N; s += kObsThreads) lo_v[row * N + s] = LZ;
    if (tid == 0) {
      vp[row] = 0.f;
      lo_u[row] = logf(fmaxf((1.f - 0.f) / (float)N, FLT_MIN));
    }
    if (prob)
      for (int i = tid; i < P; i += kObsThreads) prob[row * P + i] = -1.f;
    if (info && tid < kThr + 2) info[row * (kThr + 2) + tid] = tid == 0 ? -1 : 0;
    if (posd)
      for (long i = tid; i < (long)P * kThr; i += kObsThreads) posd[row * P * kThr + i] = -1;
    return;
  }
  for (int i = tid; i < P; i += kObsThreads) { h[i] = dn[row * P + i]; pi[i] = -1.f; }
  for (int s = tid; s < N; s += kObsThreads) own[s] = -1;
  for (int i = tid; i < nE; i += kObsThreads) { sE[i] = E[i]; sC[i] = C[i]; }
  if (tid < kThr) { sthr[tid] = thr[tid]; sbp[tid] = bp[tid]; }
  __syncthreads();
  // troughs: periods 2 tid and 2 tid + 1
  bool fl[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int i = 2 * tid + e;
    bool f = false;
    if (i < P) {
      const float v = h[i];
      if (i == 0) f = v < h[1];
      else if (i == P - 1) f = v < h[P - 2];
      else f = v < h[i - 1] && v <= h[i + 1];
    }
    fl[e] = f;
  }
  int nT;
  int at = py_block_excl_scan((int)fl[0] + (int)fl[1], wtot, tid, &nT);
#pragma unroll
  for (int e = 0; e < 2; ++e)
    if (fl[e]) { tr_i[at] = 2 * tid + e; tr_h[at] = h[2 * tid + e]; ++at; }
  __syncthreads();
  const int q = tid;
  const bool active = q < nT;
  const float hq = active ? tr_h[q] : INFINITY;
  for (int k = 0; k < kThr; ++k) {
    const unsigned long long m = __ballot(active && hq < sthr[k]);
    if (lane == 0) cnt[wave][k] = __popcll(m);
  }
  __syncthreads();
  if (tid < kThr) {
    int run = 0;
#pragma unroll
    for (int w2 = 0; w2 < kObsThreads / 64; ++w2) { const int c = cnt[w2][tid]; cnt[w2][tid] = run; run += c; }
    cnt[kObsThreads / 64][tid] = run;
  }
  __syncthreads();
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  float p = 0.f;
  int nbelow = 0;
  for (int k = 0; k < kThr; ++k) {
    const bool below = active && hq < sthr[k];
    const unsigned long long m = __ballot(below);
    int pos = -1;
    if (below) {
      pos = cnt[wave][k] + __popcll(m & lt);
      p = p + (sE[pos] * sC[cnt[kObsThreads / 64][k]]) * sbp[k];
      ++nbelow;
    }
    if (posd && active) posd[(row * P + tr_i[q]) * kThr + k] = (short)pos;
  }
  // g: the lowest trough of minimal height
  float mh = hq;
  int mq = active ? q : INT_MAX;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float oh = __shfl_xor(mh, o, 64);
    const int oq = __shfl_xor(mq, o, 64);
    if (oq != INT_MAX && (mq == INT_MAX || oh < mh || (oh == mh && oq < mq))) { mh = oh; mq = oq; }
  }
  if (lane == 0) { wminh[wave] = mh; wminq[wave] = mq; }
  __syncthreads();
  mh = wminh[0]; mq = wminq[0];
#pragma unroll
  for (int w2 = 1; w2 < kObsThreads / 64; ++w2) {
    const float oh = wminh[w2];
    const int oq = wminq[w2];
    if (oq != INT_MAX && (mq == INT_MAX || oh < mh)) { mh = oh; mq = oq; }      // later waves hold larger q: ties stay
  }
  const int m_g = kThr - nbelow;
  if (active && q == mq) {
    p = p + 0.01f * bpc[m_g];
    if (info) { info[row * (kThr + 2)] = tr_i[q]; info[row * (kThr + 2) + 1] = m_g; }
  }
  if (info) {
    if (tid == 0 && nT == 0) { info[row * (kThr + 2)] = -1; info[row * (kThr + 2) + 1] = 0; }
    if (tid < kThr) info[row * (kThr + 2) + 2 + tid] = cnt[kObsThreads / 64][tid];
  }
  if (active) {
    tr_p[q] = p;
    const int i = tr_i[q];
    pi[i] = p;
    if (p > 0.f) {
      // the shift and the bin are formed in fp64 from the fp32 dn: three-term differences of fp32 numbers cancel
      double shift = 0.0;
      if (i > 0 && i < P - 1) {
        const double l = (double)h[i - 1], c = (double)h[i], r = (double)h[i + 1];
        const double a2 = l + r - 2.0 * c, b2 = (r - l) / 2.0;
        if (fabs(b2) < fabs(a2)) shift = -b2 / a2;
      }
      const double f0 = sr / ((double)(pmin + i) + shift);
      const double v = 120.0 * log2(f0 / fmin) + 0.5;
      if (v < (double)N) {                                              // NaN and bin > N - 1: dropped
        const int bin = v < 0.0 ? 0 : min((int)floor(v), N - 1);
        atomicMax(&own[bin], q);                                        // q ascends with the period: the larger i wins
      }
    }
  }
  __syncthreads();
  if (prob)
    for (int i = tid; i < P; i += kObsThreads) prob[row * P + i] = pi[i];
  if (posd)
    for (int i = tid; i < P; i += kObsThreads)
      if (pi[i] == -1.f)                                                // no trough (a trough's p is >= 0)
        for (int k = 0; k < kThr; ++k) posd[(row * P + i) * kThr + k] = -1;
  float sum = 0.f;
  for (int s = tid; s < N; s += kObsThreads) {
    const int o = own[s];
    const float obs = o >= 0 ? tr_p[o] : 0.f;
    sum += obs;
    lo_v[row * N + s] = obs > 0.f ? logf(fmaxf(obs, FLT_MIN)) : LZ;
  }
  sum = ft_wave_sum(sum);
  if (lane == 0) wsum[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < kObsThreads / 64; ++w2) tot += wsum[w2];
    const float v = fminf(fmaxf(tot, 0.f), 1.f);
    vp[row] = v;
    lo_u[row] = logf(fmaxf((1.f - v) / (float)N, FLT_MIN));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// stage 3.  One workgroup of 1024 threads per item.  Thread tid owns state tid; the states from 1024 on (2N = 1038 at the
// shipped config: fourteen; always unvoiced ones, since N <= 1024) are spread over the waves, wave w lane i owning state
// 1024 + w + 16 i, and a wave takes the band maximum of such a state with all its lanes.  Per step: threads k < N publish
// a_v[k] and a_u[k] (the switch maximum minus lognorm, for voiced and for unvoiced targets) from delta -- these two
// arrays are delta's second buffer --, every state takes the band maximum over one of them (2 half + 1 LDS words), a
// block maximum normalises.  Three barriers a step.  With the band known at compile time (HC = half > 0) the triangle's
// logarithms sit in registers and the maximum is taken in chunks of eight, the winning chunk rescanned for its lowest
// maximal entry; otherwise they are read from LDS one by one.  Both give the maximum and the lowest source attaining it.
// Back-pointers: 16-bit source states in the workspace; backtracking at the end of the same launch, R rows at a time
// copied into LDS and walked by one thread.
// LDS: delta [2N] | a_v [N + 2 half] | a_u [N + 2 half] | red [16] f32 | redi [16] i32 | logtri [band] | from_u_v [N],
// from_u_u [N] bytes | rows [R][2N] u16
__device__ __forceinline__ float py_block_max(float v, float* red, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float m = red[0];
#pragma unroll
  for (int w = 1; w < kVitThreads / 64; ++w) {
    const float u = red[w];
    m = u > m ? u : m;
  }
  return m;
}

constexpr int kHalfShipped = 25;            // half at hop 256 / 22,050 Hz: the band the kernel is specialised for
struct VitGeom { size_t flag_off, rows_off, bytes; int R; };
__host__ __device__ inline VitGeom py_vit_geom(int N, int half) {
  VitGeom g;
  g.flag_off = ((size_t)2 * N + 2 * ((size_t)N + 2 * half) + 32 + (2 * half + 1)) * sizeof(float);
  g.rows_off = (g.flag_off + 2 * (size_t)N + 3) & ~(size_t)3;
  const size_t row = (size_t)2 * N * sizeof(unsigned short);
  const long r = g.rows_off < kLdsBudget ? (long)((kLdsBudget - g.rows_off) / row) : 0;
  g.R = (int)(r > 32 ? 32 : r);
  g.bytes = g.rows_off + (size_t)(g.R > 0 ? g.R : 0) * row;
  return g;
}

template <int HC>
__global__ __launch_bounds__(kVitThreads) void py_viterbi_kernel(
    const float* __restrict__ lo_v, const float* __restrict__ lo_u, const long* __restrict__ frames, int Tmax, int N,
    int half_arg, const float* __restrict__ logtri, const float* __restrict__ lognorm, const float* __restrict__ freqs,
    float ls, float lw, float LZ, float lN, int* __restrict__ state, float* __restrict__ score, float* __restrict__ pitch,
    unsigned short* __restrict__ back) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = HC > 0 ? HC : half_arg;
  const int S = 2 * N, NP = N + 2 * half, band = 2 * half + 1;
  const VitGeom g = py_vit_geom(N, half);
  float* dl = lds;
  float* av = dl + S;
  float* au = av + NP;
  float* red = au + NP;
  int* redi = reinterpret_cast<int*>(red + 16);
  float* lt = red + 32;
  unsigned char* fuv = reinterpret_cast<unsigned char*>(lds) + g.flag_off;
  unsigned char* fuu = fuv + N;
  unsigned short* rows = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(lds) + g.rows_off);
  const int T = (int)ft_item_len(frames, b, 1, Tmax, nullptr);
  const float* lv = lo_v + (long)b * Tmax * N;
  const float* lu = lo_u + (long)b * Tmax;
  unsigned short* bk = back + (long)b * Tmax * S;
  int* st_out = state + (long)b * Tmax;
  for (int i = tid; i < NP; i += kVitThreads)
    if (i < half || i >= half + N) { av[i] = -INFINITY; au[i] = -INFINITY; }
  for (int j = tid; j < band; j += kVitThreads) lt[j] = logtri[j];
  constexpr int BC = HC > 0 ? 2 * HC + 1 : 1;
  float ltr[BC];
  if (HC > 0) {
#pragma unroll
    for (int j = 0; j < BC; ++j) ltr[j] = logtri[j];
  }
  // this thread's states: tid, and 1024 + wave + 16 lane
  const int own[2] = {tid, kVitThreads + wave + 16 * lane};
  int sp[2];
  bool has[2], voiced[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    has[e] = own[e] < S;
    voiced[e] = own[e] < N;
    sp[e] = has[e] ? (voiced[e] ? own[e] : own[e] - N) : 0;
  }
  const float ln = tid < N ? lognorm[tid] : 0.f;
  float val[2], lo[2];
  float tmax = -INFINITY;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    val[e] = -INFINITY;
    if (has[e]) {
      val[e] = voiced[e] ? LZ + lv[sp[e]] : lN + lu[0];
      tmax = val[e] > tmax ? val[e] : tmax;
    }
  }
  float mx = py_block_max(tmax, red, tid);
  float sc = mx;
#pragma unroll
  for (int e = 0; e < 2; ++e)
    if (has[e]) dl[own[e]] = val[e] - mx;
#pragma unroll
  for (int e = 0; e < 2; ++e) lo[e] = (has[e] && T > 1) ? (voiced[e] ? lv[(long)N + sp[e]] : lu[1]) : 0.f;
  __syncthreads();
  for (int t = 1; t < T; ++t) {
    if (tid < N) {
      const float xv = dl[tid], xu = dl[N + tid];
      const float pv = xv + ls, pu = xu + lw;
      const bool f1 = pu > pv;
      av[half + tid] = (f1 ? pu : pv) - ln;
      fuv[tid] = f1;
      const float qv = xv + lw, qu = xu + ls;
      const bool f2 = qu > qv;
      au[half + tid] = (f2 ? qu : qv) - ln;
      fuu[tid] = f2;
    }
    __syncthreads();
    const float cur[2] = {lo[0], lo[1]};
    if (t + 1 < T) {                                                    // the next step's observations, ahead of their use
#pragma unroll
      for (int e = 0; e < 2; ++e)
        if (has[e]) lo[e] = voiced[e] ? lv[(long)(t + 1) * N + sp[e]] : lu[t + 1];
    }
    tmax = -INFINITY;
    if (has[0]) {
      const float* a = (voiced[0] ? av : au) + sp[0];
      float best = -INFINITY;
      int arg = half;                                                   // k = sp: always inside [0, N)
      if (HC > 0) {
        constexpr int CH = 8, NC = (BC + CH - 1) / CH;
        int argc = -1;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          float m = -INFINITY;
#pragma unroll
          for (int jj = 0; jj < CH; ++jj)
            if (c * CH + jj < BC) m = fmaxf(m, a[c * CH + jj] + ltr[c * CH + jj]);
          if (m > best) { best = m; argc = c; }
        }
        if (argc >= 0) {
#pragma unroll
          for (int jj = CH - 1; jj >= 0; --jj) {
            const int j = argc * CH + jj;
            if (j < BC && a[j] + lt[j] == best) arg = j;
          }
        }
      } else {
#pragma unroll 4
        for (int j = 0; j < band; ++j) {
          const float v = a[j] + lt[j];
          if (v > best) { best = v; arg = j; }
        }
      }
      const int k = sp[0] - half + arg;
      const int src = k + ((voiced[0] ? fuv[k] : fuu[k]) ? N : 0);
      bk[(long)t * S + tid] = (unsigned short)src;
      val[0] = best + cur[0];
      tmax = val[0];
    }
    for (int i = 0; kVitThreads + wave + 16 * i < S; ++i) {             // the wave's states beyond 1024, all lanes on each
      const int s = kVitThreads + wave + 16 * i, bin = s - N;
      float bv = -INFINITY;
      int bj = INT_MAX;
      for (int j = lane; j < band; j += 64) {
        const float v = au[bin + j] + lt[j];
        if (v > bv) { bv = v; bj = j; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (oj != INT_MAX && (bj == INT_MAX || ov > bv || (ov == bv && oj < bj))) { bv = ov; bj = oj; }
      }
      if (lane == i) {
        const int k = bin - half + (bj == INT_MAX ? half : bj);
        bk[(long)t * S + s] = (unsigned short)(k + (fuu[k] ? N : 0));
        val[1] = bv + cur[1];
        tmax = val[1] > tmax ? val[1] : tmax;
      }
    }
    mx = py_block_max(tmax, red, tid);
    sc = sc + mx;
#pragma unroll
    for (int e = 0; e < 2; ++e)
      if (has[e]) dl[own[e]] = val[e] - mx;
    __syncthreads();
  }
  // the lowest maximal final state
  int cand = INT_MAX;
#pragma unroll
  for (int e = 0; e < 2; ++e)
    if (has[e] && val[e] == mx) cand = min(cand, own[e]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
  if (lane == 0) redi[wave] = cand;
  __threadfence();
  __syncthreads();
  int s = INT_MAX;
#pragma unroll
  for (int w = 0; w < kVitThreads / 64; ++w) s = min(s, redi[w]);
  if (s >= S) s = 0;                                                    // NaN everywhere: no state equals the maximum
  if (tid == 0) {
    score[b] = sc;
    st_out[T - 1] = s;
  }
  const int words = S / 2;                                              // a row of back-pointers as 32-bit words
  for (int hi = T - 1; hi >= 1; hi -= g.R) {
    const int cnt = min(g.R, hi);                                       // rows hi, hi - 1, ..., hi - cnt + 1
    for (int i = tid; i < cnt * words; i += kVitThreads) {
      const int r = i / words, c = i - r * words;
      reinterpret_cast<unsigned*>(rows)[r * words + c] = reinterpret_cast<const unsigned*>(bk + (long)(hi - r) * S)[c];
    }
    __syncthreads();
    if (tid == 0) {
      for (int r = 0; r < cnt; ++r) {
        s = rows[r * S + s];
        s = s < S ? s : S - 1;
        st_out[hi - r - 1] = s;
      }
    }
    __syncthreads();
  }
  __threadfence();
  __syncthreads();
  for (int t = tid; t < Tmax; t += kVitThreads) {
    float f = 0.f;
    if (t < T) {
      const int q = st_out[t];
      f = q < N ? freqs[q] : 0.f;
    } else {
      st_out[t] = -1;
    }
    pitch[(long)b * Tmax + t] = f;
  }
}

bool py_cmnd_ok(int fl, int hop, int pmin, int pmax) {
  return fl >= 4 && fl % 2 == 0 && fl <= 65536 && hop >= 1 && hop <= 65536 && pmin >= 1 && pmax >= pmin + 2 &&
         pmax <= fl - fl / 2 - 1;
}
size_t py_cmnd_lds(int fl, int hop, int pmax) {
  const CmndGeom g = py_cmnd_geom(fl, hop, pmax);
  return ((size_t)g.span + (size_t)kFrames * g.DP) * sizeof(float);
}

}  // namespace

extern "C" {

size_t ft_pyin_cmnd_lds(int frame_length, int hop, int pmin, int pmax) {
  if (!py_cmnd_ok(frame_length, hop, pmin, pmax)) return 0;
  return py_cmnd_lds(frame_length, hop, pmax);
}

int ft_pyin_cmnd(const float* wav, long ld, const long* wav_len, int B, long Lmax, int frame_length, int hop, int pmin,
                 int pmax, int Tmax, float* dn, long* frames, void* stream) {
  FT_REQUIRE(B >= 0 && B <= 65535, "pyin_cmnd: bad batch size %d", B);
  if (B == 0) return FT_OK;
  FT_REQUIRE(py_cmnd_ok(frame_length, hop, pmin, pmax),
             "pyin_cmnd: frame_length %d (even, >= 4), hop %d, periods %d..%d (pmin >= 1, pmax >= pmin + 2, pmax <= "
             "frame_length - frame_length / 2 - 1)", frame_length, hop, pmin, pmax);
  const size_t lds = py_cmnd_lds(frame_length, hop, pmax);
  FT_REQUIRE(lds <= kLdsBudget, "pyin_cmnd: frame_length %d with hop %d needs %zu bytes of LDS (at most %zu)", frame_length,
             hop, lds, kLdsBudget);
  FT_REQUIRE(Lmax >= 0 && Lmax <= ld && ld >= 1 && Lmax < (1L << 40), "pyin_cmnd: Lmax (%ld) must be in 0..ld (%ld)", Lmax, ld);
  FT_REQUIRE(Tmax == 1 + Lmax / hop && (long)Tmax * (pmax - pmin + 1) < (1L << 31), "pyin_cmnd: Tmax (%d) must be 1 + Lmax / hop",
             Tmax);
  FT_REQUIRE(wav && wav_len && dn && frames, "pyin_cmnd: a null pointer");
  const dim3 grid(ft_cdiv(Tmax, kFrames), B);
  const bool vec = hop % 4 == 0 && (frame_length / 2) % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(py_cmnd_kernel<true>, grid, dim3(kCmndThreads), lds, (hipStream_t)stream, wav, ld, wav_len, Lmax,
                       frame_length, hop, pmin, pmax, Tmax, dn, frames);
  else
    hipLaunchKernelGGL(py_cmnd_kernel<false>, grid, dim3(kCmndThreads), lds, (hipStream_t)stream, wav, ld, wav_len, Lmax,
                       frame_length, hop, pmin, pmax, Tmax, dn, frames);
  return ft_check_launch("pyin_cmnd");
}

int ft_pyin_observe(const float* dn, const long* frames, int B, int Tmax, int P, int pmin, int N, double sr, double fmin,
                    const float* thr, const float* bp, const float* bpc, const float* E, const float* C, int nE, float LZ,
                    float* lo_v, float* lo_u, float* vp, float* prob, int* info, short* pos, void* stream) {
  FT_REQUIRE(B >= 0 && B <= 65535, "pyin_observe: bad batch size %d", B);
  if (B == 0) return FT_OK;
  FT_REQUIRE(P >= 3 && P <= kMaxP && pmin >= 1, "pyin_observe: P (%d) must be in 3..%d", P, kMaxP);
  FT_REQUIRE(N >= 1 && N <= kMaxN, "pyin_observe: N (%d) must be in 1..%d", N, kMaxN);
  FT_REQUIRE(nE >= (P + 1) / 2 + 1 && nE <= kMaxP / 2 + 1, "pyin_observe: the E and C tables must hold (P + 1) / 2 + 1 = %d entries",
             (P + 1) / 2 + 1);
  FT_REQUIRE(Tmax >= 1 && sr > 0 && fmin > 0, "pyin_observe: bad Tmax, sr or fmin");
  FT_REQUIRE(dn && frames && thr && bp && bpc && E && C && lo_v && lo_u && vp, "pyin_observe: a null pointer");
  hipLaunchKernelGGL(py_observe_kernel, dim3(Tmax, B), dim3(kObsThreads), 0, (hipStream_t)stream, dn, frames, Tmax, P, pmin,
                     N, sr, fmin, thr, bp, bpc, E, C, nE, LZ, lo_v, lo_u, vp, prob, info, pos);
  return ft_check_launch("pyin_observe");
}

int ft_pyin_viterbi_rows(int N, int half) {
  if (N < 1 || N > kMaxN || half < 0 || half > kMaxHalf) return 0;
  const int R = py_vit_geom(N, half).R;
  return R > 0 ? R : 0;
}

size_t ft_pyin_viterbi_workspace(int B, int Tmax, int N) {
  if (B < 1 || Tmax < 1 || N < 1 || N > kMaxN) return 0;
  return (size_t)B * Tmax * 2 * N * sizeof(unsigned short);
}

int ft_pyin_viterbi(const float* lo_v, const float* lo_u, const long* frames, int B, int Tmax, int N, int half,
                    const float* logtri, const float* lognorm, const float* freqs, float ls, float lw, float LZ, float lN,
                    int* state, float* score, float* pitch, void* ws, size_t ws_bytes, void* stream) {
  FT_REQUIRE(B >= 0 && B <= 65535, "pyin_viterbi: bad batch size %d", B);
  if (B == 0) return FT_OK;
  FT_REQUIRE(N >= 1 && N <= kMaxN, "pyin_viterbi: N (%d) must be in 1..%d (2N states, two per thread of 1024)", N, kMaxN);
  FT_REQUIRE(half >= 0 && half <= kMaxHalf, "pyin_viterbi: half (%d) must be in 0..%d", half, kMaxHalf);
  const VitGeom g = py_vit_geom(N, half);
  FT_REQUIRE(g.R >= 1, "pyin_viterbi: N %d with half %d does not fit the LDS plan", N, half);
  FT_REQUIRE(Tmax >= 1, "pyin_viterbi: bad Tmax %d", Tmax);
  FT_REQUIRE(lo_v && lo_u && frames && logtri && lognorm && freqs && state && score && pitch, "pyin_viterbi: a null pointer");
  FT_REQUIRE(ws && ws_bytes >= ft_pyin_viterbi_workspace(B, Tmax, N) && ((uintptr_t)ws) % 4 == 0,
             "pyin_viterbi: the workspace must hold ft_pyin_viterbi_workspace(B, Tmax, N) bytes");
  if (half == kHalfShipped)                                             // the shipped hop and rate: the band in registers
    hipLaunchKernelGGL(py_viterbi_kernel<kHalfShipped>, dim3(B), dim3(kVitThreads), g.bytes, (hipStream_t)stream, lo_v,
                       lo_u, frames, Tmax, N, half, logtri, lognorm, freqs, ls, lw, LZ, lN, state, score, pitch,
                       (unsigned short*)ws);
  else
    hipLaunchKernelGGL(py_viterbi_kernel<0>, dim3(B), dim3(kVitThreads), g.bytes, (hipStream_t)stream, lo_v, lo_u, frames,
                       Tmax, N, half, logtri, lognorm, freqs, ls, lw, LZ, lN, state, score, pitch, (unsigned short*)ws);
  return ft_check_launch("pyin_viterbi");
}

}  // extern "C"
