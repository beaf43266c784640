// Audio front end on the GPU: wav -> trimmed, peak-normalised wav -> log-mel (reference: utils/dsp.py:62-78,96-104
// DSP.wav_to_mel / normalize / trim_silence and the audio half of preprocess.py:78-89 Preprocessor._convert_file).
// The windowed DFT of every frame of a ragged batch is ONE ft_linear_fwd-shaped GEMM that reads the packed, padded
// signals in place with a row stride of hop samples (as vocoder.GriffinLim.stft does for one signal); this file holds
// what surrounds it, all HBM-bound, all with a fixed summation order and no atomics:
//   ft_wav_trim_peak : (1) sum of squares and max |y| of every 512-sample block of every item (one wave per block,
//                      the samples are read once); (2) one workgroup per item: frame mean squares (a 2048-sample frame
//                      centred on f*512 is four blocks), their maximum, the first / last frame above -top_db, and the
//                      peak over [start, end) -- start is a multiple of 512 and end is one or the item's length, so the
//                      peak is the maximum of whole blocks and the samples are not read again.  An item sees its own
//                      blocks only: its result does not depend on its neighbours in the batch.
//   ft_wav_pack      : cut, scale ((y / peak) * 0.95f, two fp32 operations, IEEE division) and pad (zero or reflect)
//                      every item into one buffer with a per-item stride that is a multiple of hop, and write the
//                      zero-padded trimmed wavs [B, ldw].
//   ft_mel_project   : split spectrum [rows, 2Fp] -> magnitude -> mel -> log(max(., 1e-5)) -> [B, n_mels, Tmax], pad
//                      value beyond mel_len[b].  A tile of TT frames' magnitudes is staged in LDS; the triangular mel
//                      basis is consumed SPARSE (per filter: first bin, bin count, weights; 2F weights in all instead of
//                      n_mels * F), summed over ascending bins; lanes run along t, so the stores are the transpose.
#include <math.h>

#include "ft_common.h"

namespace {

constexpr int kTrimFrame = 2048, kTrimHop = 512;

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (cdiv(nblk, 16), B), 256 threads: wave w takes blocks (blockIdx.x * 4 + w) * 4 .. + 3, two 16-byte loads per
// lane and block, all eight issued before the first use.  Samples at or beyond len[b] count as zero.
__global__ __launch_bounds__(256) void ft_wav_block_stats_kernel(const float* __restrict__ wav, long ld, long Lmax,
                                                                 const long* __restrict__ len, float* __restrict__ sq,
                                                                 float* __restrict__ mx, int nblk) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long L = ft_item_len(len, b, 0, Lmax, nullptr);
  const float* y = wav + (long)b * ld;
  const int k0 = (blockIdx.x * 4 + w) * 4;
  f32x4 v[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long s = (long)(k0 + i) * kTrimHop + h * 256 + lane * 4;
      v[i][h] = (k0 + i < nblk && s < L) ? *reinterpret_cast<const f32x4*>(y + s) : f32x4{0.f, 0.f, 0.f, 0.f};   // ld % 4 == 0
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float s2 = 0.f, m = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long s = (long)(k0 + i) * kTrimHop + h * 256 + lane * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = (s + e < L) ? v[i][h][e] : 0.f;
        s2 += x * x;
        m = fmaxf(m, fabsf(x));
      }
    }
    s2 = ft_wave_sum(s2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
    if (lane == 0 && k0 + i < nblk) {
      sq[(long)b * nblk + k0 + i] = s2;
      mx[(long)b * nblk + k0 + i] = m;
    }
  }
}

// one workgroup per item
__global__ __launch_bounds__(256) void ft_wav_trim_kernel(const float* __restrict__ sq, const float* __restrict__ mx,
                                                          int nblk, const long* __restrict__ len, long ld, int do_trim,
                                                          float top_db, int peak_norm, int hop, long* trim_start,
                                                          long* trim_end, long* wav_len, long* mel_len, float* peak,
                                                          int* scaled) {
  __shared__ double redd[256];
  __shared__ int redlo[256], redhi[256];
  __shared__ long bounds[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long L = ft_item_len(len, b, 0, ld, nullptr);
  const float* s = sq + (long)b * nblk;
  if (do_trim) {
    const int nfr = 1 + (int)(L / kTrimHop);
    auto frame_ms = [&](int f) {
      double a = 0.0;
#pragma unroll
      for (int k = f - 2; k <= f + 1; ++k)
        if (k >= 0 && k < nblk) a += (double)s[k];
      return a / kTrimFrame;
    };
    double m = 0.0;
    for (int f = tid; f < nfr; f += 256) m = fmax(m, frame_ms(f));
    redd[tid] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) redd[tid] = fmax(redd[tid], redd[tid + o]);
      __syncthreads();
    }
    const double ref_db = 10.0 * log10(fmax(1e-10, redd[0]));
    int lo = 0x7fffffff, hi = -1;
    for (int f = tid; f < nfr; f += 256)
      if (10.0 * log10(fmax(1e-10, frame_ms(f))) - ref_db > -(double)top_db) {
        lo = min(lo, f);
        hi = max(hi, f);
      }
    redlo[tid] = lo;
    redhi[tid] = hi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) {
        redlo[tid] = min(redlo[tid], redlo[tid + o]);
        redhi[tid] = max(redhi[tid], redhi[tid + o]);
      }
      __syncthreads();
    }
    if (tid == 0) {
      const bool any = redhi[0] >= 0;
      bounds[0] = any ? (long)redlo[0] * kTrimHop : 0;
      bounds[1] = any ? min(L, ((long)redhi[0] + 1) * kTrimHop) : 0;
    }
  } else if (tid == 0) {
    bounds[0] = 0;
    bounds[1] = L;
  }
  __syncthreads();
  const long st = bounds[0], en = bounds[1];
  const int kb0 = (int)(st / kTrimHop), kb1 = (int)((en + kTrimHop - 1) / kTrimHop);      // st % 512 == 0; en % 512 == 0 or en == L
  float pk = 0.f;
  for (int k = kb0 + tid; k < kb1 && k < nblk; k += 256) pk = fmaxf(pk, mx[(long)b * nblk + k]);
  __syncthreads();
  redd[tid] = (double)pk;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) redd[tid] = fmax(redd[tid], redd[tid + o]);
    __syncthreads();
  }
  if (tid == 0) {
    pk = (float)redd[0];
    trim_start[b] = st;
    trim_end[b] = en;
    wav_len[b] = en - st;
    mel_len[b] = en > st ? 1 + (en - st) / hop : 0;
    peak[b] = pk;
    scaled[b] = (peak_norm > 0 || (peak_norm == 0 && pk > 1.0f)) ? 1 : 0;
  }
}

// grid (cdiv(stride + tail, 1024), B): four consecutive samples of the packed buffer per thread.  Position p of item b
// is sample j = p - pad of its trimmed wav: the wav itself for 0 <= j < n, the padding elsewhere (zero, or the wav
// mirrored about its first / last sample).  The last item also writes the tail (zeros) that the last GEMM rows read.
__global__ __launch_bounds__(256) void ft_wav_pack_kernel(const float* __restrict__ wav, long ld,
                                                          const long* __restrict__ trim_start,
                                                          const long* __restrict__ trim_end,
                                                          const float* __restrict__ peak, const int* __restrict__ scaled,
                                                          float* __restrict__ packed, long stride, int pad, int reflect,
                                                          long tail, float* __restrict__ wav_out, long ldw, int B) {
  const int b = blockIdx.y;
  const long p = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  const long span = stride + (b == B - 1 ? tail : 0);
  if (p >= span) return;
  const long st = clampl(trim_start[b], 0, ld);
  const long n = clampl(trim_end[b], st, ld) - st;
  const float* y = wav + (long)b * ld + st;
  const float pk = peak[b];
  const bool sc = scaled[b] != 0;
  const long j0 = p - pad;
  f32x4 v, o;
  if (j0 >= 0 && j0 + 4 <= n && ((st + j0) & 3) == 0) {
    v = *reinterpret_cast<const f32x4*>(y + j0);
    if (sc)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (v[e] / pk) * 0.95f;
    o = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long j = j0 + e;
      long idx = -1;
      if (j >= 0 && j < n) idx = j;
      else if (reflect && j < 0) idx = -j;                                  // j in [-pad, 0)
      else if (reflect && j < n + pad) idx = 2 * (n - 1) - j;               // j in [n, n + pad)
      float x = 0.f;
      if (idx >= 0 && idx < n) {
        x = y[idx];
        if (sc) x = (x / pk) * 0.95f;
      }
      v[e] = x;
      o[e] = (j >= 0 && j < n) ? x : 0.f;
    }
  }
  *reinterpret_cast<f32x4*>(packed + (long)b * stride + p) = v;        // stride % 4 == 0
  if (j0 >= 0 && j0 + 4 <= ldw) *reinterpret_cast<f32x4*>(wav_out + (long)b * ldw + j0) = o;   // pad % 4 == 0, ldw % 4 == 0
}

// grid (cdiv(Tmax, TT), B), 256 threads, dynamic LDS: mag [TT][Fp + 1] | weights [nnz].  meta [n_mels][3] = first
// bin, bin count, offset into the weights.
template <int TT>
__global__ __launch_bounds__(256) void ft_mel_project_kernel(const float* __restrict__ spec, long ld_spec, int Fp,
                                                             long rows_per_item, const long* __restrict__ mel_len,
                                                             const float* __restrict__ w, const int* __restrict__ meta,
                                                             int nnz, int n_mels, int Tmax, int log_clip,
                                                             float pad_value, float* __restrict__ mel) {
  extern __shared__ float lds[];
  const int ldm = Fp + 1;                   // odd: the TT lanes of one filter sit on TT different banks
  float* mag = lds;
  float* wl = lds + TT * ldm;
  const int b = blockIdx.y, t0 = blockIdx.x * TT, tid = threadIdx.x;
  const long ml = ft_item_len(mel_len, b, 0, rows_per_item < Tmax ? rows_per_item : (long)Tmax, nullptr);
  const int nt = ml - t0 < TT ? (int)(ml - t0) : TT;
  if (nt > 0) {
    for (int i = tid; i < nnz; i += 256) wl[i] = w[i];
    const int F4 = Fp / 4, total = nt * F4;
    const float* base = spec + ((long)b * rows_per_item + t0) * ld_spec;
#pragma unroll 4
    for (int i = tid; i < total; i += 256) {
      const int t = i / F4, k = (i - t * F4) * 4;
      const f32x4 re = *reinterpret_cast<const f32x4*>(base + (long)t * ld_spec + k);
      const f32x4 im = *reinterpret_cast<const f32x4*>(base + (long)t * ld_spec + Fp + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) mag[t * ldm + k + e] = sqrtf(re[e] * re[e] + im[e] * im[e]);
    }
    __syncthreads();
  }
  const int t = tid % TT;
  if (t0 + t >= Tmax) return;
  for (int m = tid / TT; m < n_mels; m += 256 / TT) {
    float out = pad_value;
    if (t < nt) {
      int k0 = meta[3 * m], cnt = meta[3 * m + 1], wo = meta[3 * m + 2];
      if (k0 < 0 || wo < 0) cnt = 0;
      cnt = min(cnt, min(Fp - k0, nnz - wo));
      const float* mg = mag + t * ldm + k0;
      float acc = 0.f;
      for (int i = 0; i < cnt; ++i) acc = fmaf(wl[wo + i], mg[i], acc);
      out = log_clip ? logf(acc < 1e-5f ? 1e-5f : acc) : acc;        // np.clip: a NaN stays a NaN (fmaxf would drop it)
    }
    mel[((long)b * n_mels + m) * Tmax + t0 + t] = out;
  }
}

}  // namespace

extern "C" {

size_t ft_wav_trim_peak_workspace(int B, long Lmax) {
  if (B <= 0 || Lmax <= 0) return 0;
  return (size_t)2 * B * ft_cdiv(Lmax, kTrimHop) * sizeof(float);
}

int ft_wav_trim_peak(const float* wav, long ld, const long* len, int B, long Lmax, int do_trim, float top_db,
                     int peak_norm, int hop, long* trim_start, long* trim_end, long* wav_len, long* mel_len, float* peak,
                     int* scaled, void* ws, void* stream) {
  FT_REQUIRE(B >= 0 && B <= 65535, "wav_trim_peak: bad batch size %d", B);
  if (B == 0) return FT_OK;
  FT_REQUIRE(ld >= 4 && ld % 4 == 0 && ((uintptr_t)wav) % 16 == 0,
             "wav_trim_peak: the wav rows must be 16-byte aligned (ld = %ld)", ld);
  FT_REQUIRE(Lmax >= 1 && Lmax <= ld && Lmax < (1L << 40), "wav_trim_peak: Lmax (%ld) must be in 1..ld (%ld)", Lmax, ld);
  FT_REQUIRE(hop >= 1 && ws != nullptr, "wav_trim_peak: bad hop or no workspace");
  const int nblk = ft_cdiv(Lmax, kTrimHop);
  float* sq = (float*)ws;
  float* mx = sq + (long)B * nblk;
  hipLaunchKernelGGL(ft_wav_block_stats_kernel, dim3(ft_cdiv(nblk, 16), B), dim3(256), 0, (hipStream_t)stream, wav, ld,
                     Lmax, len, sq, mx, nblk);
  hipLaunchKernelGGL(ft_wav_trim_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, sq, mx, nblk, len, Lmax, do_trim,
                     top_db, peak_norm, hop, trim_start, trim_end, wav_len, mel_len, peak, scaled);
  return ft_check_launch("wav_trim_peak");
}

int ft_wav_pack(const float* wav, long ld, const long* trim_start, const long* trim_end, const float* peak,
                const int* scaled, int B, float* packed, long stride, int n_fft, int reflect, float* wav_out, long ldw,
                void* stream) {
  FT_REQUIRE(B >= 0 && B <= 65535, "wav_pack: bad batch size %d", B);
  if (B == 0) return FT_OK;
  FT_REQUIRE(n_fft >= 8 && n_fft % 8 == 0, "wav_pack: n_fft (%d) must be a multiple of 8", n_fft);
  FT_REQUIRE(ld >= 4 && ld % 4 == 0 && ldw >= 4 && ldw % 4 == 0 && stride % 4 == 0 && ((uintptr_t)wav) % 16 == 0 &&
                 ((uintptr_t)packed) % 16 == 0 && ((uintptr_t)wav_out) % 16 == 0,
             "wav_pack: rows must be 16-byte aligned (ld %ld, ldw %ld, stride %ld)", ld, ldw, stride);
  FT_REQUIRE(stride >= ldw + n_fft, "wav_pack: stride (%ld) must cover ldw + n_fft (%ld)", stride, ldw + n_fft);
  hipLaunchKernelGGL(ft_wav_pack_kernel, dim3(ft_cdiv(stride + n_fft, 1024), B), dim3(256), 0, (hipStream_t)stream, wav,
                     ld, trim_start, trim_end, peak, scaled, packed, stride, n_fft / 2, reflect, (long)n_fft, wav_out,
                     ldw, B);
  return ft_check_launch("wav_pack");
}

int ft_mel_project(const float* spec, long ld_spec, int Fp, long rows_per_item, const long* mel_len, const float* w,
                   const int* meta, int nnz, int n_mels, int B, int Tmax, int log_clip, float pad_value, float* mel,
                   void* stream) {
  FT_REQUIRE(B >= 0 && B <= 65535 && Tmax >= 0 && n_mels >= 1, "mel_project: bad dims");
  if (B == 0 || Tmax == 0) return FT_OK;
  FT_REQUIRE(Fp >= 4 && Fp % 4 == 0 && ld_spec >= 2L * Fp && ld_spec % 4 == 0 && ((uintptr_t)spec) % 16 == 0,
             "mel_project: the spectrum must be [rows, 2 Fp] with Fp %% 4 == 0 and 16-byte aligned rows");
  FT_REQUIRE(nnz >= 1 && rows_per_item >= 1, "mel_project: bad basis or row count");
  const size_t per_t = (size_t)(Fp + 1) * sizeof(float), wb = (size_t)nnz * sizeof(float);
  const dim3 block(256);
#define FT_MEL_LAUNCH(TT_)                                                                                         \
  hipLaunchKernelGGL(ft_mel_project_kernel<TT_>, dim3(ft_cdiv(Tmax, TT_), B), block, TT_ * per_t + wb,             \
                     (hipStream_t)stream, spec, ld_spec, Fp, rows_per_item, mel_len, w, meta, nnz, n_mels, Tmax,   \
                     log_clip, pad_value, mel)
  if (16 * per_t + wb <= 65536) FT_MEL_LAUNCH(16);
  else if (8 * per_t + wb <= 65536) FT_MEL_LAUNCH(8);
  else if (4 * per_t + wb <= 65536) FT_MEL_LAUNCH(4);
  else FT_REQUIRE(false, "mel_project: %d frequency columns do not fit the LDS tile", Fp);
#undef FT_MEL_LAUNCH
  return ft_check_launch("mel_project");
}

}  // extern "C"
