// Speaker embeddings on the GPU: what surrounds the GEMMs and the three LSTM-256 recurrences of speaker.VoiceEncoder
// (the algorithm is resemblyzer's published one, written out in DESIGN.md section 7, "Speaker embedding").  All of it is
// HBM-bound, with a fixed summation order, no atomics and no cross-workgroup waits:
//   ft_spk_gain              : one workgroup per item: mean square (fp64 partial sums in a fixed order that depends on the
//                              item's length alone), the increase-only gain, the item's partial count and the number of
//                              mel frames its partials cover -- both derived from the length ON THE DEVICE by the slice
//                              rule below, so a device-side length sizes nothing on the host.
//   ft_spk_pack              : gain * wav, centred (n_fft / 2 zeros in front), zero-extended, at a fixed stride per item.
//   ft_spk_mel_power         : split spectrum [rows, 2 Fp] -> power -> sparse mel basis -> [rows, n_mels] frame-major,
//                              zero rows at and past an item's frame count.
//   ft_spk_gather_partials   : (item, first frame) slots -> time-major [T, P, n_mels]; a slot the item's length does not
//                              reach is zero.
//   ft_spk_segment_mean_norm : rows -> (optionally each / its 2-norm) -> per segment: sum in ascending order / count /
//                              2-norm.  Partials -> utterance and utterances -> speaker.
// Every exclusion is a select, never a multiplication by zero: NaN in another item or beyond a length reaches nothing.
#include <math.h>

#include "ft_common.h"

namespace {

struct SpkSlices { long count, frames; };

// compute_partial_slices on the device: n samples -> the number of partials and the mel frames they cover.
// n_frames = ceil((n + 1) / hop); steps = max(1, n_frames - pf + step + 1); one slice per i in range(0, steps, step);
// the last is dropped if (n - start) / (stop - start) < cov_num / cov_den and it is not the only one.
__host__ __device__ inline SpkSlices spk_slices(long n, int hop, int pf, int step, long cov_num, long cov_den) {
  const long n_frames = (n + hop) / hop;
  long steps = n_frames - pf + step + 1;
  if (steps < 1) steps = 1;
  long k = (steps + step - 1) / step;
  const long start = (k - 1) * step * hop, len = (long)pf * hop;
  if (k > 1 && (n - start) * cov_den < cov_num * len) --k;
  return {k, (k - 1) * step + pf};
}

// one workgroup per item.  Thread tid sums the squares of samples 4 (tid + 256 i) .. + 3, i ascending, in fp64 (a product
// of two fp32 values is exact there); the 256 partial sums are added by a fixed tree.
__global__ __launch_bounds__(256) void ft_spk_gain_kernel(const float* __restrict__ wav, long ld,
                                                          const long* __restrict__ len, long Lmax, double target, int hop,
                                                          int pf, int step, long cov_num, long cov_den, int normalize,
                                                          float* __restrict__ gain, long* __restrict__ n_partials,
                                                          long* __restrict__ frames, int* err) {
  __shared__ double red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long L = ft_item_len(len, b, 1, Lmax, tid == 0 ? err : nullptr);
  const float* y = wav + (long)b * ld;
  double acc = 0.0;
  if (normalize)
    for (long j = (long)tid * 4; j < L; j += 1024) {
      if (j + 4 <= L) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + j);          // ld % 4 == 0
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += (double)v[e] * (double)v[e];
      } else {
        for (int e = 0; e < 4; ++e)
          if (j + e < L) acc += (double)y[j + e] * (double)y[j + e];
      }
    }
  red[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double ms = red[0] / (double)L;
    float g = 1.0f;
    if (normalize && ms > 0.0) {                      // ms == 0 (or NaN): gain 1
      const float c = (float)(target / sqrt(ms));     // one rounding
      g = c > 1.0f ? c : 1.0f;                        // increase only
    }
    gain[b] = g;
    const SpkSlices s = spk_slices(L, hop, pf, step, cov_num, cov_den);
    n_partials[b] = s.count;
    frames[b] = s.frames;
  }
}

// grid (cdiv(stride + tail, 1024), B): four consecutive samples of the packed buffer per thread
__global__ __launch_bounds__(256) void ft_spk_pack_kernel(const float* __restrict__ wav, long ld,
                                                          const long* __restrict__ len, long Lmax,
                                                          const float* __restrict__ gain, float* __restrict__ packed,
                                                          long stride, int pad, long tail, int B) {
  const int b = blockIdx.y;
  const long p = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p >= stride + (b == B - 1 ? tail : 0)) return;
  const long n = ft_item_len(len, b, 1, Lmax, nullptr);
  const float* y = wav + (long)b * ld;
  const float g = gain[b];
  const long j0 = p - pad;
  f32x4 v;
  if (j0 >= 0 && j0 + 4 <= n) {
    v = *reinterpret_cast<const f32x4*>(y + j0);                         // pad % 4 == 0, ld % 4 == 0
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= g;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long j = j0 + e;
      v[e] = (j >= 0 && j < n) ? y[j] * g : 0.f;
    }
  }
  *reinterpret_cast<f32x4*>(packed + (long)b * stride + p) = v;          // stride % 4 == 0
}

// grid (cdiv(rows_per_item, 16), B), 256 threads, dynamic LDS: power [16][Fp + 1] | weights [nnz]
constexpr int kMelTT = 16;
__global__ __launch_bounds__(256) void ft_spk_mel_power_kernel(const float* __restrict__ spec, long ld_spec, int Fp,
                                                               int rows_per_item, const long* __restrict__ frames,
                                                               const float* __restrict__ w, const int* __restrict__ meta,
                                                               int nnz, int n_mels, float* __restrict__ mel) {
  extern __shared__ float lds[];
  const int ldm = Fp + 1;
  float* pw = lds;
  float* wl = lds + kMelTT * ldm;
  const int b = blockIdx.y, t0 = blockIdx.x * kMelTT, tid = threadIdx.x;
  const long fr = ft_item_len(frames, b, 0, rows_per_item, nullptr);
  const int nt = fr - t0 < kMelTT ? (int)(fr - t0) : kMelTT;                // frames of this tile that exist
  const int tile = rows_per_item - t0 < kMelTT ? rows_per_item - t0 : kMelTT;
  if (nt > 0) {
    for (int i = tid; i < nnz; i += 256) wl[i] = w[i];
    const int F4 = Fp / 4, total = nt * F4;
    const float* base = spec + ((long)b * rows_per_item + t0) * ld_spec;
    for (int i = tid; i < total; i += 256) {
      const int t = i / F4, k = (i - t * F4) * 4;
      const f32x4 re = *reinterpret_cast<const f32x4*>(base + (long)t * ld_spec + k);
      const f32x4 im = *reinterpret_cast<const f32x4*>(base + (long)t * ld_spec + Fp + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) pw[t * ldm + k + e] = re[e] * re[e] + im[e] * im[e];
    }
    __syncthreads();
  }
  float* out = mel + ((long)b * rows_per_item + t0) * n_mels;
  for (int i = tid; i < tile * n_mels; i += 256) {                       // lanes run along m: frame-major stores
    const int t = i / n_mels, m = i - t * n_mels;
    float acc = 0.f;
    if (t < nt) {
      int k0 = meta[3 * m], cnt = meta[3 * m + 1], wo = meta[3 * m + 2];
      if (k0 < 0 || wo < 0) cnt = 0;
      cnt = min(cnt, min(Fp - k0, nnz - wo));
      const float* pg = pw + t * ldm + k0;
      for (int j = 0; j < cnt; ++j) acc = fmaf(wl[wo + j], pg[j], acc);
    }
    out[i] = acc;
  }
}

// one thread per element of out [T, P, n_mels]
__global__ __launch_bounds__(256) void ft_spk_gather_kernel(const float* __restrict__ mel, int rows_per_item, int n_mels,
                                                            const long* __restrict__ frames,
                                                            const int* __restrict__ table, int P, int T, int B,
                                                            float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = i / n_mels;
  if (row >= (long)T * P) return;
  const int m = (int)(i - row * n_mels), t = (int)(row / P), p = (int)(row - (long)t * P);
  const int item = table[2 * p], f0 = table[2 * p + 1];
  float v = 0.f;
  if (item >= 0 && item < B && f0 >= 0) {
    const long fr = ft_item_len(frames, item, 0, rows_per_item, nullptr);
    if ((long)f0 + T <= fr) v = mel[((long)item * rows_per_item + f0 + t) * n_mels + m];
  }
  out[i] = v;
}

// one workgroup per segment; thread e owns columns e, e + 256, ...  Row norms (normalize_rows) are one wave per row.
__global__ __launch_bounds__(256) void ft_spk_segment_kernel(const float* __restrict__ rows, int N, int E,
                                                             const long* __restrict__ index,
                                                             const long* __restrict__ offsets,
                                                             const long* __restrict__ count, int normalize_rows,
                                                             float* __restrict__ out, float* __restrict__ rows_out) {
  extern __shared__ float lds[];                      // inverse row norms [chunk of 64 rows]
  __shared__ float red[256];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  long lo = offsets[s], hi = offsets[s + 1];
  lo = lo < 0 ? 0 : lo;
  if (index == nullptr && hi > N) hi = N;
  long cnt = hi > lo ? hi - lo : 0;
  if (count != nullptr) {
    const long c = count[s];
    cnt = c < 0 ? 0 : (c < cnt ? c : cnt);
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};                // E <= 1024
  for (long c0 = 0; c0 < cnt; c0 += 64) {
    const int nc = cnt - c0 < 64 ? (int)(cnt - c0) : 64;
    if (normalize_rows) {
      __syncthreads();
      for (int r = wv; r < nc; r += 4) {
        long src = index ? index[lo + c0 + r] : lo + c0 + r;
        src = src < 0 ? 0 : (src >= N ? N - 1 : src);
        float q = 0.f;
        for (int e = lane; e < E; e += 64) {
          const float x = rows[src * E + e];
          q = fmaf(x, x, q);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        if (lane == 0) lds[r] = sqrtf(q);
      }
      __syncthreads();
    }
    for (int r = 0; r < nc; ++r) {                    // ascending rows
      long src = index ? index[lo + c0 + r] : lo + c0 + r;
      src = src < 0 ? 0 : (src >= N ? N - 1 : src);
      const float nrm = normalize_rows ? lds[r] : 1.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = tid + 256 * q;
        if (e < E) {
          float x = rows[src * E + e];
          if (normalize_rows) {
            x = x / nrm;
            if (rows_out) rows_out[src * E + e] = x;
          }
          acc[q] += x;
        }
      }
    }
  }
  float sq = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc[q] = acc[q] / (float)cnt;                     // an empty segment: 0 / 0 = NaN, as the definition says
    if (tid + 256 * q < E) sq = fmaf(acc[q], acc[q], sq);
  }
  red[tid] = sq;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const float nrm = sqrtf(red[0]);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + 256 * q;
    if (e < E) out[(long)s * E + e] = acc[q] / nrm;
  }
}

}  // namespace

extern "C" {

int ft_spk_slices(long n, int hop, int partial_frames, int frame_step, long cov_num, long cov_den, long* count,
                  long* frames) {
  FT_REQUIRE(n >= 1 && n < (1L << 40) && hop >= 1 && partial_frames >= 1 && frame_step >= 1 && cov_num >= 0 &&
                 cov_den >= 1 && cov_den <= (1L << 20) && cov_num <= cov_den,
             "spk_slices: bad arguments");
  const SpkSlices s = spk_slices(n, hop, partial_frames, frame_step, cov_num, cov_den);
  if (count) *count = s.count;
  if (frames) *frames = s.frames;
  return FT_OK;
}

int ft_spk_gain(const float* wav, long ld, const long* len, int B, long Lmax, double target, int hop, int partial_frames,
                int frame_step, long cov_num, long cov_den, int normalize, float* gain, long* n_partials, long* frames,
                int* err_flag, void* stream) {
  FT_REQUIRE(B >= 0 && B <= 65535, "spk_gain: bad batch size %d", B);
  if (B == 0) return FT_OK;
  FT_REQUIRE(ld >= 4 && ld % 4 == 0 && ((uintptr_t)wav) % 16 == 0, "spk_gain: the wav rows must be 16-byte aligned (ld = %ld)",
             ld);
  FT_REQUIRE(Lmax >= 1 && Lmax <= ld && Lmax < (1L << 40), "spk_gain: Lmax (%ld) must be in 1..ld (%ld)", Lmax, ld);
  FT_REQUIRE(hop >= 1 && partial_frames >= 1 && frame_step >= 1 && cov_num >= 0 && cov_den >= 1 && cov_den <= (1L << 20) &&
                 cov_num <= cov_den,
             "spk_gain: bad slice parameters");
  FT_REQUIRE(len && gain && n_partials && frames, "spk_gain: null output or lengths");
  hipLaunchKernelGGL(ft_spk_gain_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, wav, ld, len, Lmax, target, hop,
                     partial_frames, frame_step, cov_num, cov_den, normalize, gain, n_partials, frames, err_flag);
  return ft_check_launch("spk_gain");
}

int ft_spk_pack(const float* wav, long ld, const long* len, int B, long Lmax, const float* gain, float* packed,
                long stride, int n_fft, void* stream) {
  FT_REQUIRE(B >= 0 && B <= 65535, "spk_pack: bad batch size %d", B);
  if (B == 0) return FT_OK;
  FT_REQUIRE(n_fft >= 8 && n_fft % 8 == 0, "spk_pack: n_fft (%d) must be a multiple of 8", n_fft);
  FT_REQUIRE(ld >= 4 && ld % 4 == 0 && stride >= n_fft && stride % 4 == 0 && ((uintptr_t)wav) % 16 == 0 &&
                 ((uintptr_t)packed) % 16 == 0,
             "spk_pack: rows must be 16-byte aligned (ld %ld, stride %ld)", ld, stride);
  FT_REQUIRE(Lmax >= 1 && Lmax <= ld, "spk_pack: Lmax (%ld) must be in 1..ld (%ld)", Lmax, ld);
  hipLaunchKernelGGL(ft_spk_pack_kernel, dim3(ft_cdiv(stride + n_fft, 1024), B), dim3(256), 0, (hipStream_t)stream, wav,
                     ld, len, Lmax, gain, packed, stride, n_fft / 2, (long)n_fft, B);
  return ft_check_launch("spk_pack");
}

int ft_spk_mel_power(const float* spec, long ld_spec, int Fp, int rows_per_item, const long* frames, const float* w,
                     const int* meta, int nnz, int n_mels, int B, float* mel, void* stream) {
  FT_REQUIRE(B >= 0 && B <= 65535 && n_mels >= 1 && rows_per_item >= 1, "spk_mel_power: bad dims");
  if (B == 0) return FT_OK;
  FT_REQUIRE(Fp >= 4 && Fp % 4 == 0 && ld_spec >= 2L * Fp && ld_spec % 4 == 0 && ((uintptr_t)spec) % 16 == 0,
             "spk_mel_power: the spectrum must be [rows, 2 Fp] with Fp %% 4 == 0 and 16-byte aligned rows");
  FT_REQUIRE(nnz >= 1, "spk_mel_power: empty basis");
  const size_t lds = ((size_t)kMelTT * (Fp + 1) + nnz) * sizeof(float);
  FT_REQUIRE(lds <= 65536, "spk_mel_power: %d frequency columns do not fit the LDS tile", Fp);
  hipLaunchKernelGGL(ft_spk_mel_power_kernel, dim3(ft_cdiv(rows_per_item, kMelTT), B), dim3(256), lds,
                     (hipStream_t)stream, spec, ld_spec, Fp, rows_per_item, frames, w, meta, nnz, n_mels, mel);
  return ft_check_launch("spk_mel_power");
}

int ft_spk_gather_partials(const float* mel, int rows_per_item, int n_mels, const long* frames, const int* table, int P,
                           int partial_frames, int B, float* out, void* stream) {
  FT_REQUIRE(B >= 1 && rows_per_item >= 1 && n_mels >= 1 && P >= 0 && partial_frames >= 1, "spk_gather_partials: bad dims");
  const long total = (long)partial_frames * P * n_mels;
  if (total == 0) return FT_OK;
  FT_REQUIRE(total < (1L << 38), "spk_gather_partials: too many elements");
  hipLaunchKernelGGL(ft_spk_gather_kernel, dim3(ft_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, mel,
                     rows_per_item, n_mels, frames, table, P, partial_frames, B, out);
  return ft_check_launch("spk_gather_partials");
}

int ft_spk_segment_mean_norm(const float* rows, int N, int E, const long* index, const long* offsets, const long* count,
                             int S, int normalize_rows, float* out, float* rows_out, void* stream) {
  FT_REQUIRE(N >= 1 && E >= 1 && E <= 1024 && S >= 0 && S <= 0x7fffffff, "spk_segment_mean_norm: bad dims (N %d, E %d, S %d)",
             N, E, S);
  if (S == 0) return FT_OK;
  FT_REQUIRE(offsets != nullptr && out != nullptr, "spk_segment_mean_norm: null offsets or output");
  hipLaunchKernelGGL(ft_spk_segment_kernel, dim3(S), dim3(256), 64 * sizeof(float), (hipStream_t)stream, rows, N, E,
                     index, offsets, count, normalize_rows, out, rows_out);
  return ft_check_launch("spk_segment_mean_norm");
}

}  // extern "C"
