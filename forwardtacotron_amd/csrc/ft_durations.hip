// Duration extraction from a Tacotron attention matrix (duration_extraction/duration_extractor.py:23-84 and
// duration_extraction_pipe.py:56-62, utils/metrics.py:4-31 of the reference), one workgroup per item.
//
// The reference builds a scipy graph over the Tm x Tx cells (edges right, down and diagonal; an edge weighs the cost
// 1 - att of the cell it enters) and runs Dijkstra from cell (0,0).  The graph is a DAG whose edges all go to a later
// anti-diagonal (right / down: +1, diagonal: +2), so the same shortest distances come out of a min-plus DP swept
// anti-diagonal by anti-diagonal: on diagonal d every cell (d - j, j) is independent of the others, one lane per
// column, one barrier per diagonal.  Each cell's distance is min(dist of its three predecessors) + cost in fp64, the
// very additions Dijkstra's relaxations make (fl(a + w) is monotone in a, so the min commutes with the rounding):
// the distances equal scipy's bit for bit, and only the choice between exactly tied predecessors can differ.
//
// Tie rule (documented in forwardtacotron_amd/durations.py): diagonal, then down, then right.
//
// Back-pointers are 2 bits per cell, 16 rows of one column per 32-bit word (word (i >> 4) * Tx + j), so a word has a
// single writer: the lane that owns column j keeps it in a register and stores it once every 16 rows.  They live in
// LDS (FT_DUR_BP_LDS_WORDS words, 1250 x 200 cells fit) or, for larger items, in the global workspace.
//
// Per-item workspace row info (int4 per mel frame): x = silent flag, y = argmax over tokens of the raw attention
// (align score), z / w = first / last token the path visits in that row (the last one receives the frame).
#include "ft_common.h"
#include "fwdtaco_hip.h"

namespace {

constexpr int DUR_THREADS = 256;
constexpr int DUR_KMAX = 4;                                // columns per lane: Tx <= 1024
constexpr int DUR_TX_MAX = DUR_THREADS * DUR_KMAX;
constexpr int DUR_BP_LDS_WORDS = 28672;                    // 112 KiB of back-pointers (458,752 cells)

constexpr int DUR_ST_OK = 0, DUR_ST_XLEN = 1, DUR_ST_MELLEN = 2, DUR_ST_NOWS = 3;

__device__ __forceinline__ float dur_cell_att(float a, bool shift_row, bool sil_tok, float shift) {
  // duration_extractor.py:48-53: att_shift = sil * shift * 2 - shift, added in fp32, then clamp(0, 1)
  if (shift_row) a = a + (sil_tok ? shift : -shift);
  return fminf(fmaxf(a, 0.f), 1.f);
}

__global__ void __launch_bounds__(DUR_THREADS) ft_dur_extract_kernel(
    const float* __restrict__ attn, int Sa, int Txa, const float* __restrict__ mel, int n_mels, int Tmel,
    const long* __restrict__ x, int Txx, const long* __restrict__ x_len, const long* __restrict__ mel_len,
    const long* __restrict__ sil_ids, int n_sil, float thr, float shift, long* __restrict__ dur, int Tx_out,
    double* __restrict__ fstats, long* __restrict__ istats, int4* __restrict__ rowinfo_all,
    unsigned* __restrict__ bp_global_all) {
  __shared__ double D[3][DUR_TX_MAX + 1];                  // distances of the last three diagonals, column j at [j+1]
  __shared__ int cnt[DUR_TX_MAX];
  __shared__ double red_d[DUR_THREADS];
  __shared__ int red_i[DUR_THREADS];
  __shared__ int s_nsil, s_loc;
  __shared__ double s_cost;
  __shared__ unsigned bp_lds[DUR_BP_LDS_WORDS];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long xl_l = x_len[b], ml_l = mel_len[b];
  long* durb = dur + (long)b * Tx_out;
  int status = DUR_ST_OK;
  if (xl_l < 1 || xl_l > Txa || xl_l > Txx || xl_l > Tx_out || xl_l > DUR_TX_MAX) status = DUR_ST_XLEN;
  else if (ml_l < 1 || ml_l > Sa || ml_l > Tmel) status = DUR_ST_MELLEN;
  const int xl = (int)xl_l, ml = (int)ml_l;
  const long bp_words = (long)((ml + 15) >> 4) * xl;
  const bool bp_in_lds = bp_words <= DUR_BP_LDS_WORDS;
  if (status == DUR_ST_OK && !bp_in_lds && bp_global_all == nullptr) status = DUR_ST_NOWS;
  if (status != DUR_ST_OK) {                               // uniform over the block: nothing below runs
    for (int j = tid; j < Tx_out; j += DUR_THREADS) durb[j] = 0;
    if (tid == 0) {
      const double nan = __builtin_nan("");
      fstats[b * 3 + 0] = nan; fstats[b * 3 + 1] = nan; fstats[b * 3 + 2] = nan;
      istats[b * 3 + 0] = 0; istats[b * 3 + 1] = 0; istats[b * 3 + 2] = status;
    }
    return;
  }

  const float* A = attn + (long)b * Sa * Txa;             // A[i * Txa + j], i < ml, j < xl
  const float* M = mel + (long)b * n_mels * Tmel;          // M[c * Tmel + i]
  int4* rowinfo = rowinfo_all + (long)b * Sa;
  unsigned* bp = bp_in_lds ? bp_lds : bp_global_all + (long)b * ((Sa + 15) >> 4) * Txa;

  if (tid == 0) { s_nsil = 0; s_loc = 0; }
  for (int j = tid; j < xl; j += DUR_THREADS) cnt[j] = 0;
  __syncthreads();

  // ---- rows: silent flag (mel.mean(dim=0) < thr) and argmax of the raw attention --------------------------------
  int my_sil = 0;
  for (int i = tid; i < ml; i += DUR_THREADS) {
    // torch's column sum order for a [C, T] tensor: sequential 16-row chunks accumulated in order, the tail rows last
    float acc = 0.f;
    int c = 0;
    for (; c + 16 <= n_mels; c += 16) {
      float ch = 0.f;
      for (int k = 0; k < 16; ++k) ch += M[(long)(c + k) * Tmel + i];
      acc += ch;
    }
    float tail = 0.f;
    for (; c < n_mels; ++c) tail += M[(long)c * Tmel + i];
    acc = tail + acc;
    const int sil = (acc / (float)n_mels) < thr;
    my_sil += sil;
    rowinfo[i].x = sil;
  }
  for (int i = wave; i < ml; i += DUR_THREADS / 64) {
    float best = -__builtin_inff();
    int bi = 0x7fffffff;
    for (int j = lane; j < xl; j += 64) {
      const float v = A[(long)i * Txa + j];
      if (v > best || bi == 0x7fffffff) { best = v; bi = j; }   // first maximum of this lane's (ascending) columns
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) rowinfo[i].y = bi;
  }
  if (my_sil) atomicAdd(&s_nsil, my_sil);
  __syncthreads();

  // The reference applies the shift only if the silent frames' index list survives `nonzero().squeeze()` as a
  // list: with exactly one silent frame it is a 0-d tensor and no row is shifted (duration_extractor.py:44-46).
  const bool do_shift = s_nsil >= 2;
  {
    int loc = 0;                                           // metrics.py:19-23 with r = 1
    for (int i = 1 + tid; i < ml; i += DUR_THREADS) {
      const int d = rowinfo[i].y - rowinfo[i - 1].y;
      loc += (d >= -1 && d <= 1);
    }
    if (loc) atomicAdd(&s_loc, loc);
  }

  // ---- min-plus DP over the anti-diagonals ------------------------------------------------------------------------
  const double INF = __builtin_inf();
  bool tok_sil[DUR_KMAX];
  unsigned word[DUR_KMAX];
#pragma unroll
  for (int k = 0; k < DUR_KMAX; ++k) {
    const int j = tid + k * DUR_THREADS;
    bool s = false;
    if (j < xl) {
      const long t = x[(long)b * Txx + j];
      for (int q = 0; q < n_sil; ++q) s |= (sil_ids[q] == t);
    }
    tok_sil[k] = s;
    word[k] = 0u;
  }
  for (int j = tid; j <= xl; j += DUR_THREADS) { D[0][j] = INF; D[1][j] = INF; D[2][j] = INF; }
  __syncthreads();

  // cell (i, j) of this lane is visited on diagonal i + j; its attention and row flag are fetched one diagonal early
  float a_nx[DUR_KMAX];
  int s_nx[DUR_KMAX];
#pragma unroll
  for (int k = 0; k < DUR_KMAX; ++k) {
    const int j = tid + k * DUR_THREADS;
    a_nx[k] = 0.f; s_nx[k] = 0;
    if (j == 0) { a_nx[k] = A[0]; s_nx[k] = rowinfo[0].x; }
  }
  const int ndiag = ml + xl - 1;
  for (int d = 0; d < ndiag; ++d) {
    const int cur = d % 3, prv = (d + 2) % 3, pp = (d + 1) % 3;
#pragma unroll
    for (int k = 0; k < DUR_KMAX; ++k) {
      const int j = tid + k * DUR_THREADS;
      if (j >= xl) continue;
      const int i = d - j;
      const float a = a_nx[k];
      const int srow = s_nx[k];
      if (i + 1 >= 0 && i + 1 < ml) {                      // prefetch the cell of the next diagonal in this column
        a_nx[k] = A[(long)(i + 1) * Txa + j];
        s_nx[k] = rowinfo[i + 1].x;
      }
      double dist = INF;
      if (i >= 0 && i < ml) {
        unsigned code;
        double best;
        if (i == 0 && j == 0) { best = 0.0; code = 3u; }
        else {
          best = D[pp][j];                                 // diagonal (i-1, j-1)
          code = 0u;
          const double dn = D[prv][j + 1];                 // down from (i-1, j)
          if (dn < best) { best = dn; code = 1u; }
          const double rt = D[prv][j];                     // right from (i, j-1)
          if (rt < best) { best = rt; code = 2u; }
        }
        const float att = dur_cell_att(a, do_shift && srow, tok_sil[k], shift);
        dist = (i == 0 && j == 0) ? 0.0 : best + (double)(1.f - att);
        word[k] |= code << (2 * (i & 15));
        if ((i & 15) == 15 || i == ml - 1) {
          bp[(long)(i >> 4) * xl + j] = word[k];
          word[k] = 0u;
        }
      }
      D[cur][j + 1] = dist;
    }
    __syncthreads();
  }

  // ---- backtrack: one lane follows the pointers from (ml-1, xl-1) ---------------------------------------------------
  if (tid == 0) {
    s_cost = D[(ndiag - 1) % 3][xl];
    int i = ml - 1, j = xl - 1, jhi = j;
    while (i > 0 || j > 0) {                               // every step leaves the row or the column: <= ml + xl - 2
      unsigned code = (bp[(long)(i >> 4) * xl + j] >> (2 * (i & 15))) & 3u;
      if (i == 0) code = 2u;                               // the only move into the first row / column (the DP picks
      else if (j == 0) code = 1u;                          // it too; this only keeps NaN input inside the matrix)
      if (code == 2u) { --j; continue; }
      rowinfo[i].z = j;
      rowinfo[i].w = jhi;
      --i;
      if (code == 0u) --j;
      jhi = j;
    }
    rowinfo[0].z = 0;
    rowinfo[0].w = jhi;
  }
  __syncthreads();

  // ---- durations (each frame to the last token its row visits) and the path's mean attention over voiced frames --
  double asum = 0.0;
  int anum = 0;
  for (int i = tid; i < ml; i += DUR_THREADS) {
    const int4 r = rowinfo[i];
    atomicAdd(&cnt[r.w], 1);
    if (!r.x) {
      for (int j = r.z; j <= r.w; ++j) asum += (double)fminf(fmaxf(A[(long)i * Txa + j], 0.f), 1.f);
      anum += r.w - r.z + 1;
    }
  }
  red_d[tid] = asum;
  red_i[tid] = anum;
  __syncthreads();
  for (int j = tid; j < Tx_out; j += DUR_THREADS) durb[j] = j < xl ? (long)cnt[j] : 0;
  if (tid == 0) {
    double s = 0.0;
    long n = 0;
    for (int t = 0; t < DUR_THREADS; ++t) { s += red_d[t]; n += red_i[t]; }
    int maxd = 0, run = 0, maxrun = 0;                     // duration_extraction_pipe.py:173-183
    for (int j = 0; j < xl; ++j) {
      const int c = cnt[j];
      maxd = c > maxd ? c : maxd;
      if (c == 1) ++run;
      else { maxrun = run > maxrun ? run : maxrun; run = 0; }
    }
    maxrun = run > maxrun ? run : maxrun;
    fstats[b * 3 + 0] = n > 0 ? s / (double)n : __builtin_nan("");    // all frames silent: NaN
    fstats[b * 3 + 1] = (double)((float)s_loc / (float)(ml - 1));    // fp32 as metrics.py; ml == 1 gives NaN
    fstats[b * 3 + 2] = s_cost;
    istats[b * 3 + 0] = maxd;
    istats[b * 3 + 1] = maxrun;
    istats[b * 3 + 2] = DUR_ST_OK;
  }
}

}  // namespace

extern "C" size_t ft_dur_workspace(int B, int Tm, int Tx) {
  if (B <= 0 || Tm <= 0 || Tx <= 0) return 0;
  size_t bytes = (size_t)B * Tm * sizeof(int4);
  if ((long)((Tm + 15) >> 4) * Tx > DUR_BP_LDS_WORDS) bytes += (size_t)B * ((Tm + 15) >> 4) * Tx * sizeof(unsigned);
  return bytes;
}

extern "C" int ft_dur_extract(const float* attn, int Tm, int Tx, const float* mel, int n_mels, int Tmel, const long* x,
                              int Tx_x, const long* x_len, const long* mel_len, const long* sil_ids, int n_sil,
                              float silence_threshold, float silence_prob_shift, int B, long* durations, int Tx_out,
                              double* fstats, long* istats, void* ws, void* stream) {
  FT_REQUIRE(B >= 0 && Tm > 0 && Tx > 0 && n_mels > 0 && Tmel > 0 && Tx_x > 0 && Tx_out > 0 && n_sil >= 0,
             "dur_extract: bad dims");
  FT_REQUIRE(Tx <= DUR_TX_MAX, "dur_extract: at most %d tokens per item (got %d)", DUR_TX_MAX, Tx);
  if (B == 0) return FT_OK;
  FT_REQUIRE(ws != nullptr, "dur_extract: workspace is required");
  int4* rowinfo = (int4*)ws;
  unsigned* bpg = nullptr;
  if ((long)((Tm + 15) >> 4) * Tx > DUR_BP_LDS_WORDS) bpg = (unsigned*)((char*)ws + (size_t)B * Tm * sizeof(int4));
  hipLaunchKernelGGL(ft_dur_extract_kernel, dim3(B), dim3(DUR_THREADS), 0, (hipStream_t)stream, attn, Tm, Tx, mel,
                     n_mels, Tmel, x, Tx_x, x_len, mel_len, sil_ids, n_sil, silence_threshold, silence_prob_shift,
                     durations, Tx_out, fstats, istats, rowinfo, bpg);
  return ft_check_launch("dur_extract");
}

// ==================================================================================================================
// Per-token pitch and energy (train_tacotron.py:39-93 extract_pitch_energy, :24-35 normalize_values).
//
// ft_token_values_kernel, one workgroup per item:
//   1. frame energies, lanes over frames (loads coalesced along Tmel): sqrt(sum_c exp(mel[c,t])^2), the channels
//      added in ascending order in fp32 with each square rounded before its add (np.linalg.norm(axis=0, ord=2) is an
//      axis-0 add.reduce of the squared array); each frame's raw pitch is fetched with it, 0 past pitch_len (zeros are
//      dropped by the pitch filter, which is exactly the reference's slice truncation).  The (energy, pitch) pairs
//      live in LDS for up to TV_LDS_FRAMES frames, beyond that in the global workspace.
//   2. inclusive prefix sum of the durations in LDS (contiguous chunks per lane, a Hillis-Steele scan of the chunk
//      sums): frames [cum[j], cum[j+1]) belong to token j.
//   3. one lane per token: the segment means, accumulated in fp64 and rounded to fp32 once.
// ==================================================================================================================
namespace {

constexpr int TV_THREADS = 256;
constexpr int TV_TPL = 8;                                  // tokens per lane: Tx <= 2048
constexpr int TV_TX_MAX = TV_THREADS * TV_TPL;
constexpr int TV_LDS_FRAMES = 8192;                        // 64 KiB of (energy, pitch) pairs

constexpr int TV_ST_OK = 0, TV_ST_SUM = 1, TV_ST_XLEN = 2, TV_ST_MELLEN = 3, TV_ST_PLEN = 4, TV_ST_NEGDUR = 5,
              TV_ST_NOWS = 6;

__device__ __forceinline__ float tv_energy_term(float acc, float m) {
#pragma clang fp contract(off)
  const float e = expf(m);
  return acc + e * e;                                      // the square rounded, then the add: no FMA
}

__global__ void __launch_bounds__(TV_THREADS) ft_token_values_kernel(
    const float* __restrict__ mel, int n_mels, int Tmel, const long* __restrict__ mel_len,
    const float* __restrict__ pitch, int Tp, const long* __restrict__ pitch_len, const long* __restrict__ dur, int Tx,
    const long* __restrict__ x_len, float fmin, float fmax, float* __restrict__ pitch_tok,
    float* __restrict__ energy_tok, int* __restrict__ status, float2* __restrict__ frames_ws) {
  __shared__ float2 s_fr[TV_LDS_FRAMES];
  __shared__ long s_cum[TV_TX_MAX + 1];                    // s_cum[j + 1] = d_0 + ... + d_j, s_cum[0] = 0
  __shared__ long s_part[TV_THREADS];
  __shared__ int s_neg;

  const int b = blockIdx.x, tid = threadIdx.x;
  const long xl_l = x_len[b], ml_l = mel_len[b], pl_l = pitch_len[b];
  long d[TV_TPL];                                          // durations requested with the lengths
#pragma unroll
  for (int k = 0; k < TV_TPL; ++k) {
    const int j = tid + k * TV_THREADS;
    d[k] = j < Tx ? dur[(long)b * Tx + j] : 0;
  }
  float* pt = pitch_tok + (long)b * Tx;
  float* et = energy_tok + (long)b * Tx;

  int st = TV_ST_OK;
  if (xl_l < 1 || xl_l > Tx) st = TV_ST_XLEN;
  else if (ml_l < 1 || ml_l > Tmel) st = TV_ST_MELLEN;
  else if (pl_l < 0 || pl_l > Tp) st = TV_ST_PLEN;
  else if (ml_l > TV_LDS_FRAMES && frames_ws == nullptr) st = TV_ST_NOWS;
  if (st != TV_ST_OK) {                                    // uniform over the block
    for (int j = tid; j < Tx; j += TV_THREADS) { pt[j] = 0.f; et[j] = 0.f; }
    if (tid == 0) status[b] = st;
    return;
  }
  const int xl = (int)xl_l, ml = (int)ml_l, pl = (int)pl_l;
  float2* fr = ml <= TV_LDS_FRAMES ? s_fr : frames_ws + (long)b * Tmel;
  if (tid == 0) s_neg = 0;

  // ---- 1. frame energies and pitches --------------------------------------------------------------------------------
  const float* M = mel + (long)b * n_mels * Tmel;          // M[c * Tmel + t]
  const float* P = pitch + (long)b * Tp;
  for (int t = tid; t < ml; t += TV_THREADS) {
    const float p = t < pl ? P[t] : 0.f;
    float acc = 0.f;
    int c = 0;
    for (; c + 16 <= n_mels; c += 16) {
      float v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = M[(long)(c + k) * Tmel + t];
#pragma unroll
      for (int k = 0; k < 16; ++k) acc = tv_energy_term(acc, v[k]);
    }
    for (; c < n_mels; ++c) acc = tv_energy_term(acc, M[(long)c * Tmel + t]);
    fr[t] = make_float2(sqrtf(acc), p);
  }
  __syncthreads();                                         // s_neg initialised

  // ---- 2. duration prefix sum ---------------------------------------------------------------------------------------
  bool neg = false;
#pragma unroll
  for (int k = 0; k < TV_TPL; ++k) {
    const int j = tid + k * TV_THREADS;
    const long v = j < xl ? d[k] : 0;
    neg |= v < 0;
    s_cum[j + 1] = v;
  }
  if (neg) s_neg = 1;
  if (tid == 0) s_cum[0] = 0;
  __syncthreads();
  long part = 0;
#pragma unroll
  for (int k = 0; k < TV_TPL; ++k) part += s_cum[1 + tid * TV_TPL + k];
  s_part[tid] = part;
  __syncthreads();
  for (int o = 1; o < TV_THREADS; o <<= 1) {
    const long v = tid >= o ? s_part[tid - o] : 0;
    __syncthreads();
    s_part[tid] += v;
    __syncthreads();
  }
  long run = tid ? s_part[tid - 1] : 0;
#pragma unroll
  for (int k = 0; k < TV_TPL; ++k) {
    run += s_cum[1 + tid * TV_TPL + k];
    s_cum[1 + tid * TV_TPL + k] = run;
  }
  __syncthreads();

  // train_tacotron.py:63 asserts sum(dur) == mel_len (the item is skipped); a negative duration is an input error
  st = s_neg ? TV_ST_NEGDUR : (s_cum[xl] != ml_l ? TV_ST_SUM : TV_ST_OK);
  if (tid == 0) status[b] = st;
  if (st != TV_ST_OK) {
    for (int j = tid; j < Tx; j += TV_THREADS) { pt[j] = 0.f; et[j] = 0.f; }
    return;
  }

  // ---- 3. segment means; zip(range(mel_len), cum[:-1], cum[1:]) stops after min(mel_len, x_len) tokens --------------
  const int ntok = xl < ml ? xl : ml;
  for (int j = tid; j < Tx; j += TV_THREADS) {
    float pv = 0.f, ev = 0.f;
    if (j < ntok) {
      const int a = (int)s_cum[j], e = (int)s_cum[j + 1];  // 0 <= a <= e <= mel_len
      double ps = 0.0, es = 0.0;
      int pn = 0;
      for (int t = a; t < e; ++t) {
        const float2 f = fr[t];
        es += (double)f.x;
        if (f.y != 0.f && f.y >= fmin && f.y <= fmax) { ps += (double)f.y; ++pn; }   // NaN fails every test
      }
      if (pn) pv = (float)(ps / (double)pn);
      if (e > a) ev = (float)(es / (double)(e - a));
    }
    pt[j] = pv;
    et[j] = ev;
  }
}

// ---- per-speaker pitch statistics and normalisation (normalize_values) --------------------------------------------
// Three launches over one speaker's token pitches v[n] in the caller's (fixed) order.  Slab p covers the contiguous
// range [p * chunk, min(n, (p + 1) * chunk)), chunk = ceil(n / P), P = ps_slabs(n): a function of n only.  Every
// block that needs a total sums the P slabs itself in ascending order, so there is no atomic and no cross-workgroup
// wait, and one input gives one result bit pattern.
//   ft_pstat_sum_kernel:  slab[p] = (sum of the nonzero v, their count), fp64;
//   ft_pstat_sq_kernel:   mean = sum / count; slab[P + p].x = sum of (v - mean)^2 over the nonzero v, fp64;
//   ft_pstat_norm_kernel: std = sqrt(sq / count) (population, as np.std); mean32 = (float)mean, std32 = (float)std,
//                         std32 = 1e10 unless std32 > 0; v = (v - mean32) / std32 in fp32 where v != 0.
constexpr int PS_THREADS = 256;
constexpr int PS_MAX_SLABS = 256;
constexpr long PS_MIN_CHUNK = 4096;

int ps_slabs(long n) {
  const long p = (n + PS_MIN_CHUNK - 1) / PS_MIN_CHUNK;
  return p < 1 ? 1 : (p > PS_MAX_SLABS ? PS_MAX_SLABS : (int)p);
}

__device__ __forceinline__ double ps_block_sum(double v, double* red) {
  v = ft_wave_sum_d(v);                                    // fixed butterfly, then the four waves in order
  __syncthreads();                                         // red is free from a previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < PS_THREADS / 64; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ void ps_totals(const double2* __restrict__ slab, int P, double* sum, double* cnt,
                                          double* sq) {
  double s = 0.0, c = 0.0, q = 0.0;
  for (int p = 0; p < P; ++p) {
    const double2 a = slab[p];
    s += a.x;
    c += a.y;
    if (sq) q += slab[P + p].x;
  }
  *sum = s;
  *cnt = c;
  if (sq) *sq = q;
}

__global__ void __launch_bounds__(PS_THREADS) ft_pstat_sum_kernel(const float* __restrict__ v, long n, long chunk,
                                                                  double2* __restrict__ slab) {
  __shared__ double red[PS_THREADS / 64];
  const long lo = (long)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  double s = 0.0, c = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += PS_THREADS) {
    const float x = v[i];
    if (x != 0.f) { s += (double)x; c += 1.0; }
  }
  s = ps_block_sum(s, red);
  c = ps_block_sum(c, red);
  if (threadIdx.x == 0) slab[blockIdx.x] = make_double2(s, c);
}

__global__ void __launch_bounds__(PS_THREADS) ft_pstat_sq_kernel(const float* __restrict__ v, long n, long chunk,
                                                                 double2* __restrict__ slab) {
  __shared__ double red[PS_THREADS / 64];
  const int P = gridDim.x;
  double sum, cnt;
  ps_totals(slab, P, &sum, &cnt, nullptr);
  const double mean = sum / cnt;
  const long lo = (long)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  double q = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += PS_THREADS) {
    const float x = v[i];
    if (x != 0.f) { const double dx = (double)x - mean; q += dx * dx; }
  }
  q = ps_block_sum(q, red);
  if (threadIdx.x == 0) slab[P + blockIdx.x] = make_double2(q, 0.0);
}

__global__ void __launch_bounds__(PS_THREADS) ft_pstat_norm_kernel(float* __restrict__ v, long n, int P,
                                                                   const double2* __restrict__ slab,
                                                                   double* __restrict__ stats) {
  double sum, cnt, sq;
  ps_totals(slab, P, &sum, &cnt, &sq);
  const double mean = sum / cnt, sd = sqrt(sq / cnt);     // no nonzero value: NaN, NaN (np.mean / np.std of [])
  const float m32 = (float)mean;
  float s32 = (float)sd;
  if (!(s32 > 0.f)) s32 = 1e10f;                           // train_tacotron.py:28-29
  for (long i = (long)blockIdx.x * PS_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * PS_THREADS) {
    const float x = v[i];
    if (x != 0.f) v[i] = (x - m32) / s32;                  // zeros stay 0 (:31-34)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = cnt; stats[1] = mean; stats[2] = sd; stats[3] = (double)m32; stats[4] = (double)s32;
  }
}

}  // namespace

extern "C" size_t ft_token_values_workspace(int B, int Tmel) {
  if (B <= 0 || Tmel <= 0) return 0;
  return Tmel > TV_LDS_FRAMES ? (size_t)B * Tmel * sizeof(float2) : 0;
}

extern "C" int ft_token_values(const float* mel, int n_mels, int Tmel, const long* mel_len, const float* pitch, int Tp,
                               const long* pitch_len, const long* dur, int Tx, const long* x_len, float pitch_min_freq,
                               float pitch_max_freq, int B, float* pitch_tok, float* energy_tok, int* status, void* ws,
                               void* stream) {
  FT_REQUIRE(B >= 0 && n_mels > 0 && Tmel > 0 && Tp > 0 && Tx > 0, "token_values: bad dims");
  FT_REQUIRE(Tx <= TV_TX_MAX, "token_values: at most %d tokens per item (got %d)", TV_TX_MAX, Tx);
  if (B == 0) return FT_OK;
  FT_REQUIRE(Tmel <= TV_LDS_FRAMES || ws != nullptr, "token_values: a workspace is required for Tmel > %d",
             TV_LDS_FRAMES);
  hipLaunchKernelGGL(ft_token_values_kernel, dim3(B), dim3(TV_THREADS), 0, (hipStream_t)stream, mel, n_mels, Tmel,
                     mel_len, pitch, Tp, pitch_len, dur, Tx, x_len, pitch_min_freq, pitch_max_freq, pitch_tok,
                     energy_tok, status, Tmel > TV_LDS_FRAMES ? (float2*)ws : nullptr);
  return ft_check_launch("token_values");
}

extern "C" size_t ft_pitch_norm_workspace(long n) {
  if (n <= 0) return 0;
  return (size_t)2 * ps_slabs(n) * sizeof(double2);
}

extern "C" int ft_pitch_norm(float* values, long n, double* stats, void* ws, void* stream) {
  FT_REQUIRE(n >= 0 && stats != nullptr, "pitch_norm: bad arguments");
  if (n == 0) return FT_OK;
  FT_REQUIRE(ws != nullptr, "pitch_norm: a workspace is required");
  const int P = ps_slabs(n);
  const long chunk = (n + P - 1) / P;
  const long blocks = (n + PS_THREADS - 1) / PS_THREADS;
  double2* slab = (double2*)ws;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ft_pstat_sum_kernel, dim3(P), dim3(PS_THREADS), 0, s, values, n, chunk, slab);
  hipLaunchKernelGGL(ft_pstat_sq_kernel, dim3(P), dim3(PS_THREADS), 0, s, values, n, chunk, slab);
  hipLaunchKernelGGL(ft_pstat_norm_kernel, dim3(blocks < 1024 ? (int)blocks : 1024), dim3(PS_THREADS), 0, s, values,
                     n, P, (const double2*)slab, stats);
  return ft_check_launch("pitch_norm");
}
