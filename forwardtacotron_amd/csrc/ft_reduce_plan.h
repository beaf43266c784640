// What a column reduction will be, and how much scratch the entry points around it need, decided on the host in plain
// C++ (no HIP header, no device code, no getenv): the chunk plan of the two-stage column reductions (BatchNorm statistics
// and gradients, bias / LayerNorm column sums), the byte sizes and offsets that follow from it, the two "independent tasks
// + ordered sum" choices of the convolutions, and the three workspaces of a whole FFTBlock backward.  Every *_workspace
// query and the launcher it belongs to read ONE value from here (ft_bn.hip, ft_capi_core.hip, ft_fft_block.hip);
// tests/test_reduce_plan_cpu.py and tests/cpp/reduce_plan_main.cpp hold it to a hand-written table without a GPU.
#pragma once
#include <stddef.h>

#include "ft_gemm_plan.h"

namespace reduce_plan {

using gemm_plan::cdiv;

// ------------------------------------------------------------------------------------------------------------------
// the chunk plan: rows are cut into nchunks ranges of rows_per_chunk, one block row of partials each
struct ChunkPlan {
  int nchunks, rows_per_chunk;
};
inline ChunkPlan plan_chunks(long rows, int C) {
  int cb = cdiv(C, 64);
  // enough blocks to fill the chip, few enough chunks that the per-channel ordered finalize stays short
  long want = 1024 / (cb > 0 ? cb : 1);
  if (want < 16) want = 16;
  if (want > 64) want = 64;
  long maxc = (rows + 63) / 64;
  if (maxc < 1) maxc = 1;
  long n = want < maxc ? want : maxc;
  if (n > 65535) n = 65535;
  long rpc = (rows + n - 1) / n;
  rpc = ((rpc + 3) / 4) * 4;
  if (rpc < 4) rpc = 4;
  n = (rows + rpc - 1) / rpc;
  if (n < 1) n = 1;
  ChunkPlan p = {(int)n, (int)rpc};
  return p;
}

// one (sum0, sum1) pair of doubles per chunk and column
inline size_t partial_bytes(int nchunks, int C) { return (size_t)nchunks * C * 2 * sizeof(double); }

// the chunk plan of a column sum over [rows, C] and its scratch (an empty matrix still gets one 16-byte pair)
inline ChunkPlan colsum_chunks(long rows, int C) { return plan_chunks(rows > 0 ? rows : 1, C > 0 ? C : 1); }
inline size_t bn_bytes(long rows, int C) { return partial_bytes(plan_chunks(rows, C).nchunks, C); }
inline size_t colsum_bytes(long rows, int C) { return partial_bytes(colsum_chunks(rows, C).nchunks, C > 0 ? C : 1); }

// several column sums over matrices with the same row count in one pair of launches: every task keeps the chunking of
// its stand-alone sum, the tasks' partials lie back to back.  (The pure-arithmetic fields of the kernels' argument.)
constexpr int CSB_MAX = 16;
struct ColsumBatchLayout {
  long ws_off[CSB_MAX];                           // in doubles
  int nchunks[CSB_MAX], rpc[CSB_MAX];
  int tile64[CSB_MAX + 1], tile32[CSB_MAX + 1];   // prefix sums of the tasks' 64- / 32-column tiles
  int maxchunks;
  size_t bytes;
};
// n <= CSB_MAX
inline ColsumBatchLayout colsum_batch(int n, const int* C, long rows) {
  ColsumBatchLayout b = {};
  b.maxchunks = 1;
  for (int i = 0; i < n; ++i) {
    const ChunkPlan p = colsum_chunks(rows, C[i]);
    b.nchunks[i] = p.nchunks;
    b.rpc[i] = p.rows_per_chunk;
    b.ws_off[i] = (long)(b.bytes / sizeof(double));
    b.bytes += colsum_bytes(rows, C[i]);
    b.tile64[i + 1] = b.tile64[i] + cdiv(C[i], 64);
    b.tile32[i + 1] = b.tile32[i] + cdiv(C[i], 32);
    if (p.nchunks > b.maxchunks) b.maxchunks = p.nchunks;
  }
  return b;
}
// the size alone, for any n
inline size_t colsum_batch_bytes(int n, const int* C, long rows) {
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += colsum_bytes(rows, C[i]);
  return total;
}

// ------------------------------------------------------------------------------------------------------------------
// convolutions that leave BatchNorm statistics partials behind: the buffer holds either one partial per 128-row GEMM tile
// (statistics from the epilogue) or the chunk partials of the stand-alone pass, whichever the launch turns out to take
inline size_t conv_stats_bytes(int B, int Tbuf, int C) {
  const size_t tiles = partial_bytes(cdiv((long)B * Tbuf, 128), C);
  const size_t chunks = bn_bytes((long)B * Tbuf, C);
  return tiles > chunks ? tiles : chunks;
}

// a choice that costs scratch: taken or not, and the bytes it needs beyond what the entry point needs anyway
struct Extra {
  bool on;
  size_t extra_bytes;
};
inline Extra extra_if(bool on, size_t bytes) {
  Extra e = {on, on ? bytes : 0};
  return e;
}

// Token-side convolutions (B*T = 4096 rows) have too few 128x128 output tiles to fill the chip.  With k >= 2 taps the taps
// run as INDEPENDENT tasks of one launch -- tiles x k >= 192 workgroups, each writing its own fp32 slab -- followed by one
// ordered sum over the k slabs.  enabled: FT_CONV_TAP_SPLIT (read once by the caller).
inline Extra conv_tap_split(int B, int Tout, int Cout, int k, bool enabled) {
  const long tiles = (long)cdiv((long)B * Tout, 128) * cdiv(Cout, 128);
  const bool on = enabled && k >= 2 && k <= FT_MAX_TASKS && Cout > 64 && Cout % 4 == 0 && (long)B * Tout > 64 &&
                  tiles < 192 && tiles * k >= 192;
  return extra_if(on, (size_t)k * B * Tout * Cout * sizeof(float));
}
// ft_conv1d_fwd_stats' buffer: the statistics partials, then (256-byte aligned) the k tap slabs
struct ConvFwdStats {
  size_t stats_bytes;      // what the statistics alone need: the entry point's minimum
  size_t slab_offset;      // where the tap slabs start
  Extra tap_split;
  size_t bytes;            // the whole buffer; the taps are only split when it is all there
};
inline ConvFwdStats conv_fwd_stats(int B, int Tout, int Cout, int k, bool tap_split_enabled) {
  ConvFwdStats p;
  p.stats_bytes = conv_stats_bytes(B, Tout, Cout);
  p.slab_offset = (p.stats_bytes + 255) & ~(size_t)255;
  p.tap_split = conv_tap_split(B, Tout, Cout, k, tap_split_enabled);
  p.bytes = p.slab_offset + p.tap_split.extra_bytes;
  return p;
}

// Data gradient of a conv bank: with few output tiles a chain of the K members would leave 3/4 of the CUs idle, so there
// the members run as K independent tasks into per-member partials and an ordered sum follows.
inline Extra bank_bwd_partials(int B, int T, int Cin, int K) {
  const long tiles = (long)cdiv((long)B * T, 128) * cdiv(Cin, 128);
  const bool on = K >= 2 && Cin > 64 && (long)B * T > 64 && tiles < 192 && tiles * K >= 192;
  return extra_if(on, (size_t)K * B * T * Cin * sizeof(float));
}

// ------------------------------------------------------------------------------------------------------------------
// the three workspaces of ft_fft_blocks_bwd for a block of (B, T, d, nheads, dfft, k1, k2)
struct FftBlockPlan {
  size_t attn;        // main stream: the attention backward's row sums
  size_t tn_slabs;    // weight-gradient stream: the largest split-K slab set of the four weight gradients
  size_t sums;        // column-sum stream: the eight bias / LayerNorm sums, batched (covers the one-by-one form too: it is
                      // the sum of their sizes)
  size_t wgrad;       // a weight-gradient workspace that may also serve the sums (sums_workspace = NULL): the larger
};
inline size_t attn_bwd_bytes(int B, int T, int nheads) { return (size_t)B * nheads * T * sizeof(float); }
inline FftBlockPlan fft_block(int B, int T, int d, int nheads, int dfft, int k1, int k2, const gemm_plan::Switches& sw) {
  const int rows = B * T;
  FftBlockPlan p;
  p.attn = attn_bwd_bytes(B, T, nheads);
  p.tn_slabs = gemm_plan::conv_wgrad_query_bytes(B, T, d, dfft, k1, T, sw);
  auto up = [&](size_t v) { if (v > p.tn_slabs) p.tn_slabs = v; };
  up(gemm_plan::conv_wgrad_query_bytes(B, T, dfft, d, k2, T, sw));
  up(gemm_plan::linear_wgrad_query_bytes(rows, d, d, sw));
  up(gemm_plan::linear_wgrad_query_bytes(rows, d, 3 * d, sw));
  const int C[8] = {d, d, d, dfft, d, d, d, 3 * d};
  p.sums = colsum_batch_bytes(8, C, rows);
  p.wgrad = p.tn_slabs > p.sums ? p.tn_slabs : p.sums;
  return p;
}

}  // namespace reduce_plan
