// What the fused attention kernels share (ft_attn.hip: training forward / backward with a byte mask; ft_attn_lens.hip: the
// length-aware inference forward): bf16 fragments of fp32 rows, the row-major key-block LDS tile with its row and transposed
// fragment reads, the accumulator-to-operand conversion, the key mask of one block, the online softmax of the two forward
// kernels and the float4 row store of every epilogue.
// Everything is a template or __forceinline__, in a named namespace that the two files open with a using-directive.
#pragma once
#include "ft_common.h"

namespace ft_attn_tile {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

constexpr int KB = 64;                       // keys per block
constexpr float LOG2E = 1.44269504088896341f;

__device__ __forceinline__ int crow(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

__device__ __forceinline__ bf16x8 cvt8(const float4& a, const float4& b) {
  return bf16x8{(__bf16)a.x, (__bf16)a.y, (__bf16)a.z, (__bf16)a.w, (__bf16)b.x, (__bf16)b.y, (__bf16)b.z, (__bf16)b.w};
}

// 8 consecutive floats of a row (zeros if !ok) -> one bf16 fragment
__device__ __forceinline__ bf16x8 load_frag(const float* p, bool ok) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 a = ok ? *reinterpret_cast<const float4*>(p) : z;
  const float4 b = ok ? *reinterpret_cast<const float4*>(p + 4) : z;
  return cvt8(a, b);
}

// row-major [ROWS rows][HD] bf16 tile image, row stride RS bytes (ROWS = 64 keys everywhere but in the SPLIT = 2
// instantiations of ft_attn_lens.hip, whose key blocks are 32 rows)
template <int HD, int ROWS = KB>
struct Tile {
  static constexpr int RS = HD * 2 + 16;
  static constexpr int BYTES = ROWS * RS;
  static constexpr int F4 = ROWS * HD / 4 / 256;        // float4 per thread per tile
  // global -> registers (fp32), rows beyond T read as zeros
  __device__ static void load(float4 (&r)[F4], const float* base, long ld, int row0, int T, int tid) {
#pragma unroll
    for (int i = 0; i < F4; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / (HD / 4), c4 = idx - row * (HD / 4);
      const int g = row0 + row;
      r[i] = g < T ? *reinterpret_cast<const float4*>(base + (long)g * ld + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ static void store(unsigned char* tile, const float4 (&r)[F4], int tid) {
#pragma unroll
    for (int i = 0; i < F4; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / (HD / 4), c4 = idx - row * (HD / 4);
      const bf16x4 v = {(__bf16)r[i].x, (__bf16)r[i].y, (__bf16)r[i].z, (__bf16)r[i].w};
      *reinterpret_cast<bf16x4*>(tile + row * RS + 8 * c4) = v;
    }
  }
  // A / B fragment by rows: lane (row l31, half hf) holds columns 16*ks + 8*hf .. + 7 of tile row `row`
  __device__ static bf16x8 row_frag(const unsigned char* tile, int row, int ks, int hf) {
    return *reinterpret_cast<const bf16x8*>(tile + row * RS + 32 * ks + 16 * hf);
  }
  // transposed fragment: lane (column c0 + (lane & 31), half hf) holds tile rows r0 + 8 (j >> 2) + 4 hf + (j & 3), j = 0..7
  // -- the k order of an accumulator tile used as the other operand (file header)
  __device__ static bf16x8 tr_frag(const unsigned char* tile, int r0, int c0, int lane) {
    const int g = lane >> 4, i = lane & 15;
    const int row = r0 + 4 * (g >> 1) + (i >> 2), col = c0 + 16 * (g & 1) + 4 * (i & 3);
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const unsigned char* p = tile + row * RS + 2 * col;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 8 * RS));
    const s16x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return __builtin_bit_cast(bf16x8, v);
  }
};

// registers 8s .. 8s+7 of a 32x32 accumulator tile -> the bf16 fragment of k-step s
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& a, int s) {
  return s == 0 ? bf16x8{(__bf16)a[0], (__bf16)a[1], (__bf16)a[2], (__bf16)a[3], (__bf16)a[4], (__bf16)a[5], (__bf16)a[6],
                         (__bf16)a[7]}
                : bf16x8{(__bf16)a[8], (__bf16)a[9], (__bf16)a[10], (__bf16)a[11], (__bf16)a[12], (__bf16)a[13],
                         (__bf16)a[14], (__bf16)a[15]};
}

__device__ __forceinline__ unsigned long long pad_mask64(const unsigned char* kp, int k0, int T, int lane) {
  const int k = k0 + lane;
  const bool masked = k >= T || (kp && kp[k] != 0);
  return __ballot(masked);
}

// One key block of the online softmax on the transposed score tiles x[kt][e] = key 32 kt + crow(e, hf), query l31 (KT = 2: a
// 64-key block, KT = 1: a 32-key block): scaled to the log2 domain, masked by pm (bit k = key k of the block is masked), m / l
// updated; x becomes post(p, k) of the probabilities p = exp2(x - m_new), k the key's index within the block -- the
// identity in the inference kernels, attention dropout in ft_attn_fwd_kernel (l sums the probabilities before it);
// -> the factor the accumulated output has to be rescaled by.
template <int KT, class Post>
__device__ __forceinline__ float online_softmax(f32x16 (&x)[KT], unsigned long long pm, float c, int hf, float& m, float& l,
                                                Post post) {
  float mloc = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kk = 32 * kt + crow(e, hf);
      const float v = ((pm >> kk) & 1ull) ? -INFINITY : x[kt][e] * c;
      x[kt][e] = v;
      mloc = fmaxf(mloc, v);
    }
  mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
  const float mnew = fmaxf(m, mloc);
  const float msafe = mnew == -INFINITY ? 0.f : mnew;
  const float alpha = exp2f(m - msafe);       // m = -inf: 0
  m = mnew;
  float lsum = 0.f;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float p = __builtin_amdgcn_exp2f(x[kt][e] - msafe);      // v_exp_f32 (the ocml form was 7 % of the kernel)
      lsum += p;
      x[kt][e] = post(p, 32 * kt + crow(e, hf));
    }
  l = l * alpha + lsum;
  return alpha;
}

// rows of an output from DT transposed 32x32 accumulator tiles: lane (row l31, half hf) stores f * its columns
// 32 dt + 8 g + 4 hf .. + 3 (f = 1.0f exactly: the accumulator's own bits)
template <int DT>
__device__ __forceinline__ void store_rows(float* orow, const f32x16 (&o)[DT], int hf, float f = 1.0f) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 v = make_float4(o[dt][4 * g] * f, o[dt][4 * g + 1] * f, o[dt][4 * g + 2] * f, o[dt][4 * g + 3] * f);
      *reinterpret_cast<float4*>(orow + 32 * dt + 8 * g + 4 * hf) = v;
    }
}

template <int DT>
__device__ __forceinline__ void store_zero_rows(float* orow, int hf) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<float4*>(orow + 32 * dt + 8 * g + 4 * hf) = z;
}

}  // namespace ft_attn_tile
