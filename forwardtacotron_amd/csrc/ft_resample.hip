// Sample-rate conversion of a ragged batch of wavs on the GPU (reference: utils/dsp.py:40-42 DSP.load_wav, which is
// librosa.load(path, sr=sample_rate): every file is resampled on the way in).  What is implemented is the published
// polyphase design of scipy.signal.resample_poly / librosa res_type='polyphase': a Kaiser(5.0)-windowed sinc of
// 2 * half + 1 taps, half = 10 * max(up, down), zero phase, zero padding on both sides:
//   y[n] = sum over k in [0, len), ascending, with 0 <= half + n*down - k*up <= 2*half, of h[half + n*down - k*up] * x[k]
// for n < out_len = ceil(len * up / down), one fp32 fma chain per output.
//
// Output-stationary: a workgroup owns kTile = 1024 consecutive outputs of one item, four per thread: n0 + tid + 256 e, so
// that neighbouring lanes take neighbouring outputs -- their input samples then sit about down / up apart in LDS (with
// four consecutive outputs per lane the lanes were 4 down / up apart: an 8-way bank conflict at 2:1) -- and the tile's
// outputs go through LDS into one 16-byte store per thread.
// With c = half + n*down = q*up + p, output n reads row p of the phase-major table tab [up][Tp] (tab[p][t] =
// h[p + t*up], zero where that is past the last tap) against x[q - t], t = T-1 .. 0 -- ascending k.  The first output of
// the tile fixes (q0, p0) in 64 bits; everything inside the tile is 32-bit arithmetic relative to it.  Two routes, chosen
// by the ratio alone (never by the batch), with the same fma chain and therefore the same bits:
//   LDS route : the table and the tile's input window x[q0 - (T-1) .. ] (about kTile * down / up + T samples, loaded
//               once with 16-byte loads, zeros outside [0, len)) are staged in LDS; taken when both fit 64 KiB.
//   direct    : every operand comes straight from memory through the cache (extreme ratios: the table alone is up to
//               88 KiB, or the window of 1024 outputs does not fit).
// A term is excluded by a select on t (k < 0, k >= len, tap past the filter, output past out_len), never by a multiply
// with zero, and no sample at or past len[b] is loaded: NaN or Inf in the padding or in a neighbour reaches nothing.
// What an output gets depends on (n, len[b], x[b]) alone.  No atomics, no cross-workgroup waits.
#include "ft_common.h"

namespace {

constexpr int kTile = 1024;                 // outputs per workgroup: 256 threads x 4
constexpr int kMaxRate = 1024;              // max(up, down) after the gcd
constexpr size_t kLdsBudget = 65536;

// taps per phase, the table's (odd) row stride, and the input window of one tile in samples (a multiple of 4)
struct RsGeom { int T, Tp, W, tabN; };
__host__ __device__ inline RsGeom rs_geom(int up, int down, int half) {
  RsGeom g;
  g.T = (2 * half + up) / up;                                           // ceil((2 half + 1) / up)
  g.Tp = g.T | 1;                                                       // odd: the rows of 32 phases sit on 32 banks
  g.W = ((up - 1 + (kTile - 1) * down) / up + g.T + 3 + 3) & ~3;        // + 3: the window starts on a multiple of 4
  g.tabN = (up * g.Tp + 3) & ~3;
  return g;
}

template <bool LDS>
__global__ __launch_bounds__(256) void ft_resample_kernel(const float* __restrict__ x, long ldx,
                                                          const long* __restrict__ len, long Lmax,
                                                          const float* __restrict__ tab, int up, int down, int half,
                                                          float* __restrict__ y, long ldy, long* __restrict__ out_len,
                                                          int* err) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const bool first = blockIdx.x == 0 && tid == 0;
  const long L = ft_item_len(len, b, 0, Lmax, first ? err : nullptr);
  const long nout = (L * up + down - 1) / down;
  if (first) out_len[b] = nout;
  const long n0 = (long)blockIdx.x * kTile, j0 = n0 + tid * 4;
  float* yr = y + (long)b * ldy;
  if (n0 >= nout) {                                                     // the whole tile is padding
    if (j0 < ldy) *reinterpret_cast<f32x4*>(yr + j0) = f32x4{0.f, 0.f, 0.f, 0.f};      // ldy % 4 == 0
    return;
  }
  const RsGeom g = rs_geom(up, down, half);
  const int T = g.T, Tp = g.Tp;
  const float* xr = x + (long)b * ldx;
  const long c0 = (long)half + n0 * down, q0 = c0 / up;
  const int p0 = (int)(c0 - q0 * up);
  const long kfirst = q0 - (T - 1), kb = kfirst & ~3L;                  // the window's first sample, rounded down to 4
  float* tl = lds;
  float* xw = lds + g.tabN;
  if (LDS) {
    for (int i = tid * 4; i < g.tabN; i += 1024)
      *reinterpret_cast<f32x4*>(tl + i) = *reinterpret_cast<const f32x4*>(tab + i);
    for (int i = tid * 4; i < g.W; i += 1024) {
      const long k = kb + i;
      f32x4 v;
      if (k >= 0 && k + 4 <= L) {
        v = *reinterpret_cast<const f32x4*>(xr + k);                    // ldx % 4 == 0, k % 4 == 0
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (k + e >= 0 && k + e < L) ? xr[k + e] : 0.f;
      }
      *reinterpret_cast<f32x4*>(xw + i) = v;
    }
    __syncthreads();
  }
  int cb[4], xb[4], tlo[4], thi[4];
  long qe[4];
  float acc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int m = e * 256 + tid;                                        // neighbouring lanes, neighbouring outputs
    const unsigned u = (unsigned)p0 + (unsigned)m * (unsigned)down;     // < 2^21
    const int dq = (int)(u / (unsigned)up), p = (int)(u - (unsigned)dq * (unsigned)up);
    const long q = q0 + dq;
    const int tmax = (2 * half - p) / up;                               // the last tap of phase p
    thi[e] = q < tmax ? (int)q : tmax;                                  // k = q - t >= 0
    const long lo = q - L + 1;                                          // k = q - t <= L - 1
    tlo[e] = lo < 0 ? 0 : (lo > T ? T : (int)lo);
    if (n0 + m >= nout) tlo[e] = T;                                     // past out_len: no term, exactly 0
    cb[e] = p * Tp;
    xb[e] = dq + (T - 1) + (int)(kfirst - kb);
    qe[e] = q;
    acc[e] = 0.f;
  }
#pragma unroll 4
  for (int t = T - 1; t >= 0; --t) {                                    // descending t = ascending k
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = t >= tlo[e] && t <= thi[e];
      float c, xv;
      if (LDS) {
        c = tl[cb[e] + t];
        xv = xw[xb[e] - t];
      } else {
        c = tab[cb[e] + t];
        xv = ok ? xr[qe[e] - t] : 0.f;
      }
      acc[e] = ok ? fmaf(c, xv, acc[e]) : acc[e];
    }
  }
  float* yo = LDS ? xw + g.W : lds;                                     // kTile floats of their own: no wait before the writes
#pragma unroll
  for (int e = 0; e < 4; ++e) yo[e * 256 + tid] = acc[e];
  __syncthreads();
  if (j0 < ldy) *reinterpret_cast<f32x4*>(yr + j0) = *reinterpret_cast<const f32x4*>(yo + tid * 4);
}

// up == down: the item itself, zero beyond its length
__global__ __launch_bounds__(256) void ft_resample_copy_kernel(const float* __restrict__ x, long ldx,
                                                               const long* __restrict__ len, long Lmax,
                                                               float* __restrict__ y, long ldy,
                                                               long* __restrict__ out_len, int* err) {
  const int b = blockIdx.y;
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  const long L = ft_item_len(len, b, 0, Lmax, first ? err : nullptr);
  if (first) out_len[b] = L;
  const long j = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (j >= ldy) return;
  const float* xr = x + (long)b * ldx;
  f32x4 v;
  if (j + 4 <= L) {
    v = *reinterpret_cast<const f32x4*>(xr + j);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (j + e < L) ? xr[j + e] : 0.f;
  }
  *reinterpret_cast<f32x4*>(y + (long)b * ldy + j) = v;
}

// LDS of the LDS route: table | input window | the tile's outputs
size_t rs_lds_bytes(int up, int down, int half) {
  const RsGeom g = rs_geom(up, down, half);
  return ((size_t)g.tabN + (size_t)g.W + kTile) * sizeof(float);
}
bool rs_fits_lds(int up, int down, int half) { return rs_lds_bytes(up, down, half) <= kLdsBudget; }

}  // namespace

extern "C" {

int ft_resample_table_floats(int up, int down, int half) {
  if (up < 1 || down < 1 || up > kMaxRate || down > kMaxRate || half < 0 || half > 10 * kMaxRate) return 0;
  return rs_geom(up, down, half).tabN;
}

int ft_resample_tile(int up, int down, int half) {
  if (up < 1 || down < 1 || up > kMaxRate || down > kMaxRate || half < 0 || half > 10 * kMaxRate) return 0;
  return kTile;
}

int ft_resample_route(int up, int down, int half) {
  if (up < 1 || down < 1 || up > kMaxRate || down > kMaxRate || half < 0 || half > 10 * kMaxRate) return -1;
  if (up == down) return 2;
  return rs_fits_lds(up, down, half) ? 1 : 0;
}

int ft_resample_poly_ragged(const float* x, long ldx, const long* len, int B, long Lmax, const float* tab, int up,
                            int down, int half, float* y, long ldy, long* out_len, int* err_flag, void* stream) {
  FT_REQUIRE(B >= 0 && B <= 65535, "resample_poly_ragged: bad batch size %d", B);
  if (B == 0) return FT_OK;
  FT_REQUIRE(up >= 1 && down >= 1 && up <= kMaxRate && down <= kMaxRate,
             "resample_poly_ragged: up / down = %d / %d: both must be in 1..%d", up, down, kMaxRate);
  FT_REQUIRE(half >= 0 && half <= 10 * kMaxRate, "resample_poly_ragged: half (%d) must be in 0..%d", half, 10 * kMaxRate);
  FT_REQUIRE(ldx >= 4 && ldx % 4 == 0 && ldy >= 4 && ldy % 4 == 0 && ((uintptr_t)x) % 16 == 0 && ((uintptr_t)y) % 16 == 0,
             "resample_poly_ragged: the rows must be 16-byte aligned (ldx %ld, ldy %ld)", ldx, ldy);
  FT_REQUIRE(Lmax >= 1 && Lmax <= ldx && Lmax < (1L << 40), "resample_poly_ragged: Lmax (%ld) must be in 1..ldx (%ld)", Lmax,
             ldx);
  const long nmax = (Lmax * up + down - 1) / down;
  FT_REQUIRE(ldy >= nmax && ldy < (1L << 40), "resample_poly_ragged: ldy (%ld) must hold ceil(Lmax * up / down) = %ld", ldy,
             nmax);
  FT_REQUIRE(len != nullptr && out_len != nullptr, "resample_poly_ragged: no lengths");
  const dim3 block(256);
  if (up == down) {
    hipLaunchKernelGGL(ft_resample_copy_kernel, dim3(ft_cdiv(ldy, 1024), B), block, 0, (hipStream_t)stream, x, ldx, len,
                       Lmax, y, ldy, out_len, err_flag);
    return ft_check_launch("resample_poly_ragged");
  }
  FT_REQUIRE(tab != nullptr && ((uintptr_t)tab) % 16 == 0, "resample_poly_ragged: the coefficient table must be 16-byte aligned");
  const dim3 grid(ft_cdiv(ldy, kTile), B);
  if (rs_fits_lds(up, down, half))
    hipLaunchKernelGGL(ft_resample_kernel<true>, grid, block, rs_lds_bytes(up, down, half), (hipStream_t)stream, x, ldx,
                       len, Lmax, tab, up, down, half, y, ldy, out_len, err_flag);
  else
    hipLaunchKernelGGL(ft_resample_kernel<false>, grid, block, kTile * sizeof(float), (hipStream_t)stream, x, ldx, len,
                       Lmax, tab, up, down, half, y, ldy, out_len, err_flag);
  return ft_check_launch("resample_poly_ragged");
}

}  // extern "C"
