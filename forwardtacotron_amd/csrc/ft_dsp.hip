// Mel inversion + Griffin-Lim on the GPU (reference: utils/dsp.py:80-94 DSP.griffinlim, called from gen_forward.py:109-116).
// The transforms themselves are GEMMs: a 1024-point real DFT of N windowed frames is frames[N,1024] x basis^T on the
// MFMA GEMM kernels (ft_linear_fwd; the frames are read IN PLACE out of the zero-padded signal with a row stride of
// hop samples), the inverse is proj[N,2F] x inverse-basis^T.  What is left for this file is element-wise / gather work,
// all HBM-bound:
//   ft_exp_transpose : log-mel [C,T] -> exp -> [T,C]                     (DSP.denormalize + layout for the GEMMs)
//   ft_nnls_step     : X = max(0, X - G / L)                             (projected-gradient step of the mel inversion)
//   ft_sub           : out = a - b
//   ft_gl_init       : proj = S * exp(2 pi i u)                          (random initial phases, u drawn by the host)
//   ft_gl_phase      : c = R - alpha * R_prev ; proj = S * c / (|c| + tiny) ; R_prev = R     (fast Griffin-Lim update)
//   ft_overlap_add   : y_pad[t] = sum_n frames[n][t - n*hop] * inv_wss[t]  inside [n_fft/2, n_fft/2 + L), 0 in the
//                      margins (gather form: every sample sums its <= n_fft/hop frames in a fixed order)
// Complex spectra are stored split: [N][2*Fp] = Re (Fp columns) | Im (Fp columns), Fp = F rounded up to 4.
// The *_ragged kernels do the same for a whole ragged batch in one launch each (vocoder.GriffinLim.griffinlim_batch):
// item b owns rows [b*Tcap, (b+1)*Tcap) of every frame-major buffer and samples [b*Tcap*hop, ...) of the packed signal,
// its length N_b = mel_len[b] is read on the device, rows n >= N_b are zero by SELECT (never a product with zero), and
// nothing an item gets depends on B, Tcap, Tmax or its position -- semantics in include/fwdtaco_hip.h.
#include <math.h>

#include "ft_common.h"

namespace {

__global__ __launch_bounds__(256) void ft_exp_transpose_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                               int C, int T) {
  __shared__ float tile[32][33];
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + threadIdx.x;
    tile[i][threadIdx.x] = (c < C && t < T) ? expf(in[(long)c * T + t]) : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + threadIdx.x;
    if (t < T && c < C) out[(long)t * C + c] = tile[threadIdx.x][i];
  }
}

__global__ __launch_bounds__(256) void ft_nnls_step_kernel(float* __restrict__ x, const float* __restrict__ g,
                                                           float inv_l, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = fmaxf(x[i] - inv_l * g[i], 0.f);
}

__global__ __launch_bounds__(256) void ft_sub_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     float* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = a[i] - b[i];
}

__global__ __launch_bounds__(256) void ft_gl_init_kernel(const float* __restrict__ u, const float* __restrict__ S,
                                                         float* __restrict__ proj, int N, int Fp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * Fp) return;
  const long n = i / Fp;
  const int m = (int)(i - n * Fp);
  float sn, cs;
  sincosf(6.283185307179586f * u[i], &sn, &cs);
  const float s = S[i];
  proj[n * 2 * Fp + m] = s * cs;
  proj[n * 2 * Fp + Fp + m] = s * sn;
}

__global__ __launch_bounds__(256) void ft_gl_phase_kernel(const float* __restrict__ rebuilt, float* __restrict__ tprev,
                                                          const float* __restrict__ S, float* __restrict__ proj, int N,
                                                          int Fp, float alpha, int has_prev) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * Fp) return;
  const long n = i / Fp;
  const int m = (int)(i - n * Fp);
  const long ire = n * 2 * Fp + m, iim = ire + Fp;
  const float re = rebuilt[ire], im = rebuilt[iim];
  float cr = re, cim = im;
  if (has_prev) {
    cr -= alpha * tprev[ire];
    cim -= alpha * tprev[iim];
  }
  const float inv = 1.0f / (sqrtf(cr * cr + cim * cim) + 1.17549435e-38f);
  const float s = S[i];
  proj[ire] = s * cr * inv;
  proj[iim] = s * cim * inv;
  tprev[ire] = re;
  tprev[iim] = im;
}

__global__ __launch_bounds__(256) void ft_overlap_add_kernel(const float* __restrict__ frames,
                                                             const float* __restrict__ inv_wss, float* __restrict__ ypad,
                                                             int N, int n_fft, int hop) {
  const long total = (long)n_fft + (long)hop * (N - 1);
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long pad = n_fft / 2;
  float acc = 0.f;
  if (t >= pad && t < total - pad) {
    // frames n with 0 <= t - n*hop < n_fft, ascending n (fixed order)
    long n_lo = (t - n_fft + hop) / hop;            // ceil((t - n_fft + 1) / hop) for t - n_fft + 1 > 0
    if (t - n_fft + 1 <= 0) n_lo = 0;
    long n_hi = t / hop;
    if (n_hi > N - 1) n_hi = N - 1;
    for (long n = n_lo; n <= n_hi; ++n) acc += frames[n * n_fft + (t - n * hop)];
    acc *= inv_wss[t];
  }
  ypad[t] = acc;
}

// ---- ragged batch ------------------------------------------------------------------------------------------------
// an item's frame count is ft_item_len(mel_len, b, 1, Tmax, err): clamped into [1, Tmax]
__global__ __launch_bounds__(256) void ft_gl_exp_transpose_ragged_kernel(const float* __restrict__ in,
                                                                         const long* __restrict__ mel_len,
                                                                         float* __restrict__ out, int C, int Tmax,
                                                                         int Tcap, int* err) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const bool first = (blockIdx.x | blockIdx.y | threadIdx.x | threadIdx.y) == 0;
  const int N = (int)ft_item_len(mel_len, b, 1, Tmax, first ? err : nullptr);
  const float* src = in + (long)b * C * Tmax;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + threadIdx.x;
    float v = 0.f;
    if (c < C && t < N) v = expf(src[(long)c * Tmax + t]);       // the padding of mel is never read
    tile[i][threadIdx.x] = v;
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + threadIdx.x;
    if (t < Tcap && c < C) out[((long)b * Tcap + t) * C + c] = tile[threadIdx.x][i];
  }
}

__global__ __launch_bounds__(256) void ft_gl_relu_kernel(float* __restrict__ x, long n) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 4 <= n && (((uintptr_t)x) & 15) == 0) {
    float4 v = *reinterpret_cast<float4*>(x + i);
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    *reinterpret_cast<float4*>(x + i) = v;
  } else {
    for (long j = i; j < n && j < i + 4; ++j) x[j] = fmaxf(x[j], 0.f);
  }
}

// u(seed, n, m) in [0, 1): 24 bits of ft_hash32(seed, n * Fp + m) -- keyed on the frame and the bin, not on the item
__device__ __forceinline__ float gl_draw_u(uint64_t seed, int n, int Fp, int m) {
  return (float)(ft_hash32(seed, (uint64_t)n * (uint64_t)Fp + (uint64_t)m) >> 8) * (1.0f / 16777216.0f);
}

__global__ __launch_bounds__(256) void ft_gl_init_ragged_kernel(const float* __restrict__ u, uint64_t seed,
                                                                const float* __restrict__ S,
                                                                const long* __restrict__ mel_len,
                                                                float* __restrict__ proj, float* __restrict__ u_out,
                                                                int B, int Tcap, int Tmax, int Fp, int* err) {
  const int q = Fp / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Tcap * q) return;
  const long row = i / q;
  const int m = (int)(i - row * q) * 4;
  const int b = (int)(row / Tcap), n = (int)(row - (long)b * Tcap);
  const int N = (int)ft_item_len(mel_len, b, 1, Tmax, (n == 0 && m == 0) ? err : nullptr);
  float4 re = make_float4(0.f, 0.f, 0.f, 0.f), im = re, uu = re;
  if (n < N) {
    const float4 s = *reinterpret_cast<const float4*>(S + row * Fp + m);
    if (u) uu = *reinterpret_cast<const float4*>(u + row * Fp + m);
    else uu = make_float4(gl_draw_u(seed, n, Fp, m), gl_draw_u(seed, n, Fp, m + 1), gl_draw_u(seed, n, Fp, m + 2),
                          gl_draw_u(seed, n, Fp, m + 3));
    float sn, cs;
    sincosf(6.283185307179586f * uu.x, &sn, &cs); re.x = s.x * cs; im.x = s.x * sn;
    sincosf(6.283185307179586f * uu.y, &sn, &cs); re.y = s.y * cs; im.y = s.y * sn;
    sincosf(6.283185307179586f * uu.z, &sn, &cs); re.z = s.z * cs; im.z = s.z * sn;
    sincosf(6.283185307179586f * uu.w, &sn, &cs); re.w = s.w * cs; im.w = s.w * sn;
  }
  *reinterpret_cast<float4*>(proj + row * 2 * Fp + m) = re;
  *reinterpret_cast<float4*>(proj + row * 2 * Fp + Fp + m) = im;
  if (u_out) *reinterpret_cast<float4*>(u_out + row * Fp + m) = uu;
}

__device__ __forceinline__ void gl_phase1(float re, float im, float pre, float pim, float s, float alpha, int has_prev,
                                          float* ore, float* oim) {
  float cr = re, cim = im;
  if (has_prev) {
    cr -= alpha * pre;
    cim -= alpha * pim;
  }
  const float inv = 1.0f / (sqrtf(cr * cr + cim * cim) + 1.17549435e-38f);
  *ore = s * cr * inv;
  *oim = s * cim * inv;
}

__global__ __launch_bounds__(256) void ft_gl_phase_ragged_kernel(const float* __restrict__ rebuilt,
                                                                 float* __restrict__ tprev, const float* __restrict__ S,
                                                                 const long* __restrict__ mel_len,
                                                                 float* __restrict__ proj, int B, int Tcap, int Tmax,
                                                                 int Fp, float alpha, int has_prev) {
  const int q = Fp / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Tcap * q) return;
  const long row = i / q;
  const int m = (int)(i - row * q) * 4;
  const int b = (int)(row / Tcap), n = (int)(row - (long)b * Tcap);
  const int N = (int)ft_item_len(mel_len, b, 1, Tmax, nullptr);
  const long ire = row * 2 * Fp + m, iim = ire + Fp;
  float4 pr = make_float4(0.f, 0.f, 0.f, 0.f), pi = pr, tr = pr, ti = pr;
  if (n < N) {                                  // rows past the item: `rebuilt` holds its neighbour's samples, not read
    tr = *reinterpret_cast<const float4*>(rebuilt + ire);
    ti = *reinterpret_cast<const float4*>(rebuilt + iim);
    float4 qr = pr, qi = pr;
    if (has_prev) {
      qr = *reinterpret_cast<const float4*>(tprev + ire);
      qi = *reinterpret_cast<const float4*>(tprev + iim);
    }
    const float4 s = *reinterpret_cast<const float4*>(S + row * Fp + m);
    gl_phase1(tr.x, ti.x, qr.x, qi.x, s.x, alpha, has_prev, &pr.x, &pi.x);
    gl_phase1(tr.y, ti.y, qr.y, qi.y, s.y, alpha, has_prev, &pr.y, &pi.y);
    gl_phase1(tr.z, ti.z, qr.z, qi.z, s.z, alpha, has_prev, &pr.z, &pi.z);
    gl_phase1(tr.w, ti.w, qr.w, qi.w, s.w, alpha, has_prev, &pr.w, &pi.w);
  }
  *reinterpret_cast<float4*>(proj + ire) = pr;
  *reinterpret_cast<float4*>(proj + iim) = pi;
  *reinterpret_cast<float4*>(tprev + ire) = tr;
  *reinterpret_cast<float4*>(tprev + iim) = ti;
}

__device__ __forceinline__ float gl_norm1(float acc, float ws) {
  return ws > 1.17549435e-38f ? acc * (1.0f / ws) : acc;         // the oracle's rule: no division below FLT_MIN
}

// four consecutive samples t .. t+3 (t % 4 == 0) of an item's padded signal: they share their frames because hop % 4 == 0
__device__ __forceinline__ float4 gl_ola4(const float* __restrict__ fr, const float* __restrict__ w2, int N, int n_fft,
                                          int hop, long t) {
  const long n_lo = t >= n_fft ? (t - n_fft) / hop + 1 : 0;
  long n_hi = t / hop;
  if (n_hi > N - 1) n_hi = N - 1;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), ws = acc;
  for (long n = n_lo; n <= n_hi; ++n) {         // ascending n: the fixed order of ft_overlap_add
    const long o = t - n * hop;                 // 0 <= o <= n_fft - 4
    const float4 f = *reinterpret_cast<const float4*>(fr + n * n_fft + o);
    const float4 w = *reinterpret_cast<const float4*>(w2 + o);
    acc.x += f.x; acc.y += f.y; acc.z += f.z; acc.w += f.w;
    ws.x += w.x; ws.y += w.y; ws.z += w.z; ws.w += w.w;
  }
  return make_float4(gl_norm1(acc.x, ws.x), gl_norm1(acc.y, ws.y), gl_norm1(acc.z, ws.z), gl_norm1(acc.w, ws.w));
}

__global__ __launch_bounds__(256) void ft_overlap_add_ragged_kernel(const float* __restrict__ frames,
                                                                    const float* __restrict__ w2,
                                                                    const long* __restrict__ mel_len,
                                                                    float* __restrict__ ypad, float* __restrict__ wav,
                                                                    int B, int Tcap, int Tmax, int n_fft, int hop) {
  const int b = blockIdx.y;
  const int N = (int)ft_item_len(mel_len, b, 1, Tmax, nullptr);
  const long pad = n_fft / 2, sig = (long)hop * (N - 1);        // the item's signal is ypad_b[pad, pad + sig)
  const float* fr = frames + (long)b * Tcap * n_fft;
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (wav) {                                    // last pass: the signal itself, zero beyond wav_len[b]
    const long ldw = (long)hop * (Tmax - 1);
    if (i >= ldw) return;
    if (i < sig) v = gl_ola4(fr, w2, N, n_fft, hop, pad + i);
    *reinterpret_cast<float4*>(wav + (long)b * ldw + i) = v;
  } else {                                      // the next STFT's operand; the last item also writes the n_fft zero tail
    const long stride = (long)Tcap * hop;
    if (i >= stride + (b == B - 1 ? n_fft : 0)) return;
    if (i >= pad && i < pad + sig) v = gl_ola4(fr, w2, N, n_fft, hop, i);
    *reinterpret_cast<float4*>(ypad + (long)b * stride + i) = v;
  }
}

}  // namespace

extern "C" {

int ft_exp_transpose(const float* mel_log, float* out, int C, int T, void* stream) {
  FT_REQUIRE(C >= 0 && T >= 0, "exp_transpose: bad dims");
  if (C == 0 || T == 0) return FT_OK;
  hipLaunchKernelGGL(ft_exp_transpose_kernel, dim3(ft_cdiv(T, 32), ft_cdiv(C, 32)), dim3(32, 8), 0, (hipStream_t)stream,
                     mel_log, out, C, T);
  return ft_check_launch("exp_transpose");
}

int ft_nnls_step(float* x, const float* g, float inv_l, long n, void* stream) {
  if (n <= 0) return FT_OK;
  hipLaunchKernelGGL(ft_nnls_step_kernel, dim3(ft_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, g, inv_l, n);
  return ft_check_launch("nnls_step");
}

int ft_sub(const float* a, const float* b, float* out, long n, void* stream) {
  if (n <= 0) return FT_OK;
  hipLaunchKernelGGL(ft_sub_kernel, dim3(ft_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, n);
  return ft_check_launch("sub");
}

int ft_gl_init(const float* u, const float* S, float* proj, int N, int Fp, void* stream) {
  FT_REQUIRE(N >= 0 && Fp >= 0, "gl_init: bad dims");
  if ((long)N * Fp == 0) return FT_OK;
  hipLaunchKernelGGL(ft_gl_init_kernel, dim3(ft_cdiv((long)N * Fp, 256)), dim3(256), 0, (hipStream_t)stream, u, S, proj,
                     N, Fp);
  return ft_check_launch("gl_init");
}

int ft_gl_phase(const float* rebuilt, float* tprev, const float* S, float* proj, int N, int Fp, float alpha,
                int has_prev, void* stream) {
  FT_REQUIRE(N >= 0 && Fp >= 0, "gl_phase: bad dims");
  if ((long)N * Fp == 0) return FT_OK;
  hipLaunchKernelGGL(ft_gl_phase_kernel, dim3(ft_cdiv((long)N * Fp, 256)), dim3(256), 0, (hipStream_t)stream, rebuilt,
                     tprev, S, proj, N, Fp, alpha, has_prev);
  return ft_check_launch("gl_phase");
}

int ft_overlap_add(const float* frames, const float* inv_wss, float* ypad, int N, int n_fft, int hop, void* stream) {
  FT_REQUIRE(N >= 1 && n_fft >= 2 && hop >= 1 && hop <= n_fft, "overlap_add: bad dims");
  const long total = (long)n_fft + (long)hop * (N - 1);
  hipLaunchKernelGGL(ft_overlap_add_kernel, dim3(ft_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, frames,
                     inv_wss, ypad, N, n_fft, hop);
  return ft_check_launch("overlap_add");
}

int ft_gl_exp_transpose_ragged(const float* mel, const long* mel_len, float* out, int B, int C, int Tmax, int Tcap,
                               int* err_flag, void* stream) {
  FT_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && Tmax >= 1 && Tcap >= Tmax, "gl_exp_transpose_ragged: bad dims");
  FT_REQUIRE(ft_cdiv(C, 32) <= 65535, "gl_exp_transpose_ragged: too many channels");
  hipLaunchKernelGGL(ft_gl_exp_transpose_ragged_kernel, dim3(ft_cdiv(Tcap, 32), ft_cdiv(C, 32), B), dim3(32, 8), 0,
                     (hipStream_t)stream, mel, mel_len, out, C, Tmax, Tcap, err_flag);
  return ft_check_launch("gl_exp_transpose_ragged");
}

int ft_gl_relu(float* x, long n, void* stream) {
  if (n <= 0) return FT_OK;
  hipLaunchKernelGGL(ft_gl_relu_kernel, dim3(ft_cdiv(ft_cdiv(n, 4), 256)), dim3(256), 0, (hipStream_t)stream, x, n);
  return ft_check_launch("gl_relu");
}

static int gl_ragged_dims(const char* what, int B, int Tcap, int Tmax, int Fp, const void* a, const void* b,
                          const void* c) {
  FT_REQUIRE(B >= 1 && Tmax >= 1 && Tcap >= Tmax && Fp >= 4 && Fp % 4 == 0, "%s: bad dims (Fp must be a multiple of 4)",
             what);
  FT_REQUIRE((long)B * Tcap * (Fp / 4) < (1L << 31) * 256, "%s: too many rows", what);
  FT_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0, "%s: buffers must be 16-byte aligned", what);
  return FT_OK;
}

int ft_gl_init_ragged(const float* u, uint64_t seed, const float* S, const long* mel_len, float* proj, float* u_out,
                      int B, int Tcap, int Tmax, int Fp, int* err_flag, void* stream) {
  if (gl_ragged_dims("gl_init_ragged", B, Tcap, Tmax, Fp, S, proj, u) ||
      gl_ragged_dims("gl_init_ragged", B, Tcap, Tmax, Fp, u_out, nullptr, nullptr))
    return FT_ERR_ARG;
  hipLaunchKernelGGL(ft_gl_init_ragged_kernel, dim3(ft_cdiv((long)B * Tcap * (Fp / 4), 256)), dim3(256), 0,
                     (hipStream_t)stream, u, seed, S, mel_len, proj, u_out, B, Tcap, Tmax, Fp, err_flag);
  return ft_check_launch("gl_init_ragged");
}

int ft_gl_phase_ragged(const float* rebuilt, float* tprev, const float* S, const long* mel_len, float* proj, int B,
                       int Tcap, int Tmax, int Fp, float alpha, int has_prev, void* stream) {
  if (gl_ragged_dims("gl_phase_ragged", B, Tcap, Tmax, Fp, rebuilt, tprev, S) ||
      gl_ragged_dims("gl_phase_ragged", B, Tcap, Tmax, Fp, proj, nullptr, nullptr))
    return FT_ERR_ARG;
  hipLaunchKernelGGL(ft_gl_phase_ragged_kernel, dim3(ft_cdiv((long)B * Tcap * (Fp / 4), 256)), dim3(256), 0,
                     (hipStream_t)stream, rebuilt, tprev, S, mel_len, proj, B, Tcap, Tmax, Fp, alpha, has_prev);
  return ft_check_launch("gl_phase_ragged");
}

int ft_overlap_add_ragged(const float* frames, const float* w2, const long* mel_len, float* ypad, float* wav, int B,
                          int Tcap, int Tmax, int n_fft, int hop, void* stream) {
  FT_REQUIRE(B >= 1 && B <= 65535 && Tmax >= 1 && n_fft >= 8 && n_fft % 8 == 0 && hop >= 4 && hop % 4 == 0 && hop <= n_fft,
             "overlap_add_ragged: bad dims (n_fft must be a multiple of 8, hop of 4, hop <= n_fft)");
  FT_REQUIRE((long)Tcap * hop >= (long)n_fft + (long)hop * (Tmax - 1),
             "overlap_add_ragged: an item's padded signal does not fit in its stride (Tcap %d)", Tcap);
  FT_REQUIRE((ypad != nullptr) != (wav != nullptr), "overlap_add_ragged: exactly one of ypad and wav");
  FT_REQUIRE((((uintptr_t)frames | (uintptr_t)w2 | (uintptr_t)ypad | (uintptr_t)wav) & 15) == 0,
             "overlap_add_ragged: buffers must be 16-byte aligned");
  const long span = wav ? (long)hop * (Tmax - 1) : (long)Tcap * hop + n_fft;
  if (span == 0) return FT_OK;
  hipLaunchKernelGGL(ft_overlap_add_ragged_kernel, dim3(ft_cdiv(span, 1024), B), dim3(256), 0, (hipStream_t)stream,
                     frames, w2, mel_len, ypad, wav, B, Tcap, Tmax, n_fft, hop);
  return ft_check_launch("overlap_add_ragged");
}

}  // extern "C"
