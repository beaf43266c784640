/* fwdtaco_hip.h -- C ABI of libfwdtaco_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the ForwardTacotron mel-generation hot path of ziyaad30/ForwardTacotron.
 * The reference has no FFI layer of its own (its "kernels" are stock torch.nn modules), so each entry
 * point below names the reference op it replaces (file:line relative to the reference root).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless stated; all float tensors are
 *     contiguous fp32, activations are CHANNELS-LAST  [B, T, C]  (row = one (b,t) position, `ld*` = row
 *     stride in floats) -- the reference's [B,C,T] transposes (forward_tacotron.py:32,36,134,155,...) vanish;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work (no sync, no allocation) unless
 *     stated, so they are capturable in a hipGraph -- except the recurrences (ft_gru_*, ft_lstm_*): their persistent
 *     form keeps host-side admission bookkeeping (event records / queries per launch), capture those with
 *     ft_rnn_set_persistent(0) or leave them outside the graph (tests/test_gpu_primitives.py captures a token-side chain);
 *   - return 0 on success; non-zero = error, message via ft_last_error() (thread-local);
 *   - workspaces are caller-allocated device memory, sized by the matching *_workspace() query (bytes).
 */
#ifndef FWDTACO_HIP_H
#define FWDTACO_HIP_H

#include <stddef.h>
#include <stdint.h>

#define FWDTACO_ABI_VERSION 8

#ifdef __cplusplus
extern "C" {
#endif

const char* ft_last_error(void);
int ft_abi_version(void);
/* host query: CU count and whether device 0 is gfx950 */
int ft_device_info(int* cu_count, int* is_gfx950);

/* Matmul precision of every GEMM-shaped entry point below (process-wide; returns the previous setting):
 * 0 (default) = fp32-exact (f32 MFMA, or exact three-way bf16 splits with fp32 accumulation);
 * 1 = bf16: operands rounded to nearest bf16 on load, ONE bf16 MFMA per product, fp32 accumulation, fp32 outputs --
 *     BASELINE configs[2] (FastPitch "bf16"); applies to the NT-form aligned launches (Linear / Conv1d forward, their
 *     data gradients, every weight gradient, attention Q K^T); the rest (NN-form attention products, odd shapes) and all
 *     non-GEMM kernels (LayerNorm, softmax statistics, losses, optimizer, recurrences) stay fp32. */
int ft_set_gemm_precision(int bf16);
/* weight-gradient launches that took the software-pipelined 128x128 kernel since the library loaded (tests use it to
 * prove which kernel they exercised; the choice never changes results: both kernels give the same bits) */
int ft_gemm_tn_pipelined_launches(void);
/* Launches per GEMM kernel variant since the library loaded, counted on the host where the launchers dispatch (plain
 * integers: no device work, no synchronisation).  Fills counts[0 .. min(n, FT_GEMM_VARIANTS) - 1] and returns
 * FT_GEMM_VARIANTS.  Order (forwardtacotron_amd/hip.py: GEMM_VARIANTS names them):
 *   row kernels, f32 MFMA:  0-3 the 64x64 tile as NT fast, NT not fast, NN fast, NN not fast ("fast" = 16-B loads: aligned
 *                           operands, K % 4 == 0 or padded rows); 4-7 the 128x128 tile in the same order;
 *   row kernels, bf16 split (or bf16 mode): 8 64x64, 9 128x128 two-barrier, 10 128x128 pipelined, 11 pipelined with split-K;
 *   weight gradients (TN), f32 MFMA: 12 64 fast, 13 64 not fast, 14 128 fast, 15 128 not fast;
 *   weight gradients, bf16 split (or bf16 mode): 16 64, 17 128 two-barrier, 18 128 pipelined.
 * Tests assert the delta of the one variant they mean to exercise (tests/test_gpu_gemm_edges.py). */
#define FT_GEMM_VARIANTS 19
int ft_gemm_variant_counts(long* counts, int n);

/* ---- nn.Linear (models/forward_tacotron.py:25,100,108 ; common_layers.py:31-32,83) ------------------ */
/* Row layouts: the rows of an activation matrix are the (b,t) positions in batch-major order (row = b*T+t,
 * i.e. a contiguous [B,T,C] tensor) unless a `*_tm_B` argument is > 0, in which case that operand is stored
 * TIME-major ([T,B,C], row = t*B+b, B = the argument; rows % B == 0).  The recurrences keep their buffers
 * time-major (each timestep's slab contiguous); the GEMMs read / write either order for free.
 * y[rows,out_f] (+)= x[rows,in_f] * w[out_f,in_f]^T + bias ; optional relu */
int ft_linear_fwd(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, int rows,
                  int in_f, int out_f, int relu, int accumulate, int x_tm_B, int y_tm_B, void* stream);
/* several Linear layers sharing one input, written side by side into y (highway W1|W2, RNN fwd|rev W_ih):
 * y[:, col_offset[i] : col_offset[i]+out_f[i]] = x * w[i]^T + bias[i]   (host arrays of device pointers) */
int ft_linear_multi_fwd(const float* x, long ldx, int ntasks, const float* const* w, const float* const* bias,
                        float* y, long ldy, const int* col_offset, const int* out_f, int rows, int in_f, int relu,
                        int x_tm_B, int y_tm_B, void* stream);
/* The same product, computed by the kernel that a launch over `as_rows` rows of the same layers would take
 * (the launcher picks 128x128 bf16-split or 64x64 f32 tiles by size, and the two round differently): the LengthRegulator
 * repeats rows, so a projection of its RESULT can be formed on its input with the bits the frame-level launch would give
 * every row (ops.LRBiLSTMFn). */
int ft_linear_multi_fwd_as(const float* x, long ldx, int ntasks, const float* const* w, const float* const* bias,
                           float* y, long ldy, const int* col_offset, const int* out_f, int rows, int in_f, long as_rows,
                           void* stream);
/* dx[rows,in_f] (+)= dy[rows,out_f] * w[out_f,in_f] ; w_transposed = 1: `w` points at w^T [in_f,out_f] instead
 * (both operands then have the contraction index contiguous -- the form the bf16-split MFMA kernel takes) */
int ft_linear_bwd_data(const float* dy, long lddy, const float* w, float* dx, long lddx, int rows, int in_f,
                       int out_f, int accumulate, int dy_tm_B, int dx_tm_B, int w_transposed, void* stream);
/* dw[out_f,in_f] (+)= dy^T * shift(x): rows = B*T logical positions; x_shift != 0 reads x row (b, t+x_shift),
 * zero outside [0,T) (recurrent-weight gradients: h_{t-1} / h_{t+1}); dy_time_major / x_time_major = 1 when
 * that operand is stored [T,B,*].  Deterministic split + ordered reduce. */
size_t ft_linear_bwd_weight_workspace(int rows, int in_f, int out_f);
int ft_linear_bwd_weight(const float* dy, long lddy, const float* x, long ldx, float* dw, int rows, int in_f,
                         int out_f, int B, int T, int x_shift, int accumulate, int dy_time_major, int x_time_major,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- nn.Conv1d(stride 1, padding k//2, bias=False) of BatchNormConv (common_layers.py:50,55-56) ------ */
/* weights are consumed TAP-MAJOR: wp[k][Cout][Cin] (ft_conv_pack_weight from torch's [Cout][Cin][k]).
 * y[b,t',co] = relu?( sum_j sum_ci x[b, t'+j-k/2, ci] * w[co,ci,j] ) (* scale[co] + shift[co] if scale) for
 * t' in [0,Tout); Tout = T (odd k, or even k sliced as the CBHG does, common_layers.py:99) or T+1 (even k);
 * accumulate=1 adds the result onto y (residual connection, common_layers.py:114). */
int ft_conv_pack_weight(const float* w, float* wp, int Cout, int Cin, int k, void* stream);
/* transposed tap-major pack wpt[k][Cin][Cout] for the data gradients (`wp_transposed` = 1 below): the contraction
 * index Cout becomes contiguous, which lets the gradient GEMM run in the NT form (see `w_transposed`) */
int ft_conv_pack_weight_t(const float* w, float* wpt, int Cout, int Cin, int k, void* stream);
/* All of a model's operand re-layouts in ONE launch (weights change once per optimizer step, so a training step
 * refreshes every pack / transpose up front instead of one small launch per layer).  Entry e re-lays
 * src [d0][d1][k] (a Conv1d weight [Cout][Cin][k]; a Linear / RNN weight [out_f][in_f] has k = 1) as
 * dst [k][d0][d1] (ft_conv_pack_weight) and / or dst_t [k][d1][d0] (ft_conv_pack_weight_t; the transpose of a
 * matrix); either may be NULL.  tile_begin = sum over earlier entries of k*ceil(d0/32)*ceil(d1/32), ascending;
 * `descs` is a DEVICE array of n entries, total_tiles the sum over all entries. */
typedef struct FtPackDesc {
  const float* src;
  float* dst;
  float* dst_t;
  long tile_begin;
  int d0, d1, k, reserved;
} FtPackDesc;
int ft_pack_weights(const FtPackDesc* descs, int n, long total_tiles, void* stream);
int ft_conv1d_fwd(const float* x, long ldx, const float* wp, const float* scale, const float* shift, float* y,
                  long ldy, int B, int T, int Cin, int Cout, int k, int Tout, int relu, int accumulate,
                  void* stream);
/* The eval-mode convolution of a RAGGED inference batch (ForwardTacotron.generate_batch; no reference counterpart: the
 * reference's generate, forward_tacotron.py:167-234, passes no lengths).  As ft_conv1d_fwd with Tout = T, and the
 * epilogue stores exactly 0 at rows t >= lens[b] (int64 [B], device) -- relu(conv) * scale + shift of BatchNormConv
 * (common_layers.py:55-57) is non-zero there, and the next convolution would read it across the item's end. */
int ft_conv1d_fwd_lens(const float* x, long ldx, const float* wp, const float* scale, const float* shift, float* y,
                       long ldy, const long* lens, int B, int T, int Cin, int Cout, int k, int relu, int accumulate,
                       void* stream);
/* CBHG conv1d_bank (common_layers.py:72-76,97-102): members k=1..K (K<=16) in ONE launch; member i writes
 * ybank[:, :, i*C:(i+1)*C] of ybank[B,Tout,K*C]; wp_all = packed member weights back to back. */
int ft_conv_bank_fwd(const float* x, long ldx, const float* wp_all, const float* scale, const float* shift,
                     float* ybank, int B, int T, int Cin, int C, int K, int Tout, int relu, void* stream);
/* dx[b,t,ci] (+)= sum_j sum_co dy[b, t-j+k/2, co] * w[co,ci,j]; dy is [B,Tbuf,*] of which rows < Tvalid count */
int ft_conv1d_bwd_data(const float* dy, long lddy, const float* wp, float* dx, long lddx, int B, int T, int Cin,
                       int Cout, int k, int Tbuf, int Tvalid, int accumulate, int wp_transposed, void* stream);
/* the same through a ReLU's derivative: dx[r,c] = (that product) if y[r*lddx + c] > 0 else 0, y = the OUTPUT of the conv + ReLU
 * whose result this convolution consumed (FFTBlock: conv2's data gradient is conv1's pre-ReLU gradient,
 * common_layers.py:178-180) -- the mask is the GEMM's epilogue, not an element-wise pass.  T = Tbuf = Tvalid. */
int ft_conv1d_bwd_data_relu(const float* dy, long lddy, const float* wp, const float* y, float* dx, long lddx, int B,
                            int T, int Cin, int Cout, int k, int wp_transposed, void* stream);
/* dx (+)= sum_i dy_i[rows,out_f] * w_i[out_f,in_f]: the data gradients of several nn.Linear that read the same input
 * (HighwayNetwork W1/W2, common_layers.py:35-40; the two directions' W_ih of nn.GRU / nn.LSTM) in ONE launch,
 * accumulated in registers.  dy / w: host arrays of ntasks device pointers (ntasks <= 16). */
int ft_linear_bwd_data_multi(int ntasks, const float* const* dy, long lddy, const float* const* w, float* dx, long lddx,
                             int rows, int in_f, int out_f, int accumulate, int dy_tm_B, int dx_tm_B, int w_transposed,
                             void* stream);
/* The same product with scratch for split-K (ft_linear_bwd_data_multi_workspace bytes; 0 = it would not be split): few
 * output tiles -- token-side rows -- and a long contraction leave most of the chip idle in one pass over K, so the
 * contraction is cut into up to 16 ranges whose partial tiles a second launch adds in range order.  Same products, another
 * summation order than the unsplit launch. */
size_t ft_linear_bwd_data_multi_workspace(int ntasks, int rows, int in_f, int out_f, void* stream);
int ft_linear_bwd_data_multi_ws(int ntasks, const float* const* dy, long lddy, const float* const* w, float* dx, long lddx,
                                int rows, int in_f, int out_f, int accumulate, int dy_tm_B, int dx_tm_B, int w_transposed,
                                void* workspace, size_t workspace_bytes, void* stream);
/* data gradient of the whole conv bank (backward of common_layers.py:97-102) in ONE GEMM launch; dy = [B,Tbuf,K*C]
 * gradient of the bank buffer (Tbuf = T or T+1).  Long sequences: the K members' products are accumulated in registers
 * straight into dx[B,T,Cin].  Short ones (too few output tiles to fill the chip, e.g. the prenet's B*T = 4096 rows):
 * every member writes its own partial into `workspace` (size from the query, may be 0) and an ordered sum follows. */
size_t ft_conv_bank_bwd_data_workspace(int B, int T, int Cin, int K);
int ft_conv_bank_bwd_data(const float* dy, long lddy, const float* wp_all, float* dx, long lddx, int B, int T, int Cin,
                          int C, int K, int Tbuf, int wp_transposed, void* workspace, size_t workspace_bytes,
                          void* stream);
/* weight gradients of ALL K members of a conv bank in one GEMM launch + one ordered reduction: dy [B,Tbuf,K*C] =
 * gradient of the bank buffer, x [B,T,Cin] = the bank's input, dw = HOST array of K device pointers, dw[i] =
 * torch-layout [C][Cin][i+1] gradient of member i (kernel size i+1).  C % 128 == 0. */
size_t ft_conv_bank_bwd_weight_workspace(int B, int T, int Cin, int C, int K, int Tbuf);
int ft_conv_bank_bwd_weight(const float* dy, long lddy, const float* x, long ldx, float* const* dw, int B, int T,
                            int Cin, int C, int K, int Tbuf, void* workspace, size_t workspace_bytes, void* stream);
/* dw[co,ci,j] = sum_{b,t'<Tvalid} dy[b,t',co] * x[b,t'+j-k/2,ci]   (torch layout [Cout][Cin][k]) */
size_t ft_conv1d_bwd_weight_workspace(int B, int T, int Cin, int Cout, int k, int Tvalid);
int ft_conv1d_bwd_weight(const float* dy, long lddy, const float* x, long ldx, float* dw, int B, int T, int Cin,
                         int Cout, int k, int Tbuf, int Tvalid, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- FastPitch building blocks (models/fast_pitch.py, common_layers.py:127-223) -------------------------- */
/* nn.Conv1d WITH bias, odd k, padding k//2 (FFTBlock conv1 k=9 + ReLU, conv2 k=1; common_layers.py:161-164,178-180) */
int ft_conv1d_bias_fwd(const float* x, long ldx, const float* wp, const float* bias, float* y, long ldy, int B, int T,
                       int Cin, int Cout, int k, int relu, void* stream);
/* strided-batch GEMMs for nn.MultiheadAttention (common_layers.py:158,172-174): nb0*nb1 independent instances,
 * instance z -> (z0,z1) = (z/nb1, z%nb1), operand X_z = X + z0*sX0 + z1*sX1 (floats).
 *   nt: C_z[M,N] = A_z[M,K] * B_z[N,K]^T   (scores = Q K^T ; dP = dCtx V^T)
 *   nn: C_z[M,N] = A_z[M,K] * B_z[K,N]     (ctx = P V ; dQ = dS K)
 *   tn: C_z[M,N] = A_z[R,M]^T * B_z[R,N]   (dV = P^T dCtx ; dK = dS^T Q), deterministic split + reduce
 * Row padding: attention's [T,T] matrices have a row length (841 frames) that is not a multiple of 4.  The caller keeps
 * them with a row stride rounded up to 4 and says so -- nn: a_rows_padded = 1 (every row of A readable up to the next
 * multiple of 4 of K; the values there are ignored), tn: rows_padded = 1 (rows of A / B readable up to the next multiple
 * of 4 of M / N; those columns only reach masked outputs) -- which keeps these launches on the 16-B-load paths. */
int ft_bgemm_nt(const float* A, long lda, long sA0, long sA1, const float* Bm, long ldb, long sB0, long sB1, float* C,
                long ldc, long sC0, long sC1, int M, int N, int K, int nb0, int nb1, void* stream);
int ft_bgemm_nn(const float* A, long lda, long sA0, long sA1, const float* Bm, long ldb, long sB0, long sB1, float* C,
                long ldc, long sC0, long sC1, int M, int N, int K, int nb0, int nb1, int a_rows_padded, void* stream);
size_t ft_bgemm_tn_workspace(int M, int N, int R, int nb0, int nb1);
int ft_bgemm_tn(const float* A, long lda, long sA0, long sA1, const float* Bm, long ldb, long sB0, long sB1, float* C,
                long ldc, long sC0, long sC1, int M, int N, int R, int nb0, int nb1, int rows_padded, void* workspace,
                size_t workspace_bytes, void* stream);
/* scores[B,nh,Tq,Tk] (row stride ld >= Tk floats; columns Tk..ld-1 are written as zeros) <- softmax(scale*scores +
 * mask) in place; key_pad[B,Tk] bytes (non-zero = padded key) or NULL.  dropout_p > 0 also writes dropped =
 * F.dropout(P, p) (nn.MultiheadAttention's attention dropout; same layout) with ft_dropout's counter-based mask over the
 * flat LOGICAL [B,nh,Tq,Tk] index, in the same pass. */
int ft_softmax_fwd(float* scores, const unsigned char* key_pad, int B, int nh, int Tq, int Tk, long ld, float scale,
                   float* dropped, float dropout_p, uint64_t dropout_seed, void* stream);
/* dprobs <- scale * P * (dprobs' - rowsum(dprobs'*P)) in place (pad columns -> 0); dropout_p > 0: dprobs arrives as the
 * gradient of the DROPPED probabilities and dprobs' = mask * dprobs / (1-p) is formed here (same seed as the forward) */
int ft_softmax_bwd(const float* probs, float* dprobs, int B, int nh, int Tq, int Tk, long ld, float scale, float dropout_p,
                   uint64_t dropout_seed, void* stream);
/* nn.LayerNorm(D) over the last dim with an optional fused residual add: s = x (+res) (stored to sum_out if not
 * NULL), y = LN(s); per-row mean / rstd saved.  bwd: dx (gradient wrt s) and dy_xhat = dy*xhat whose column
 * sums are dgamma (dbeta = column sums of dy), via ft_colsum. */
/* res_dropout_p > 0: the residual branch is F.dropout(res, p) computed on the fly with ft_dropout's counter-based mask
 * (seed, flat element index) -- FFTBlock's norm(src + dropout(src2)) (common_layers.py:175-176,181-183) in one pass;
 * the backward then also writes dres = d/d(res) = mask * dx / (1-p) (dres may be NULL). */
int ft_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* sum_out,
                     float* y, float* mean, float* rstd, long rows, int D, float eps, float res_dropout_p,
                     uint64_t res_dropout_seed, void* stream);
int ft_layernorm_bwd(const float* dy, const float* s, const float* gamma, const float* mean, const float* rstd,
                     float* dx, float* dy_xhat, float* dres, long rows, int D, float res_dropout_p,
                     uint64_t res_dropout_seed, void* stream);
/* PositionalEncoding (common_layers.py:127-145): out = x + scale[0]*pe[t,:]; dscale = sum(dout*pe) */
int ft_posenc_fwd(const float* x, const float* pe, const float* scale, float* out, int B, int T, int D,
                  void* stream);
size_t ft_posenc_workspace(void);
int ft_posenc_bwd_scale(const float* dout, const float* pe, float* dscale, int B, int T, int D, void* workspace,
                        size_t workspace_bytes, void* stream);
int ft_relu_bwd(const float* dy, const float* y, float* dx, long n, void* stream);

/* ---- LengthRegulator (common_layers.py:12-24) ------------------------------------------------------- */
/* scan: clamps dur[dur<0]=0 IN PLACE (as the reference does), r=(long)(dur+0.5); cum[b][0..Tx] exclusive
 * frame offsets (int32, [B,Tx+1]); total[b] = cum[b][Tx].  Caller reads max(total) to size the output. */
int ft_lr_scan(float* dur, int B, int Tx, int* cum, int* total, void* stream);
/* Durations of a ragged inference batch, per item (forward_tacotron.py:174-177 with common_layers.py:17-24 applied to
 * item b alone, L = x_len[b]): if sum_{j<L} trunc(dur[b,j]) <= 0 every token j < L gets 2.0; then, in place,
 * dur[b,j] = 0 at j >= L and negatives are clamped to 0; mel_len[b] (int64) = sum_j (long)(dur[b,j] + 0.5), the total
 * ft_lr_scan gives.  An x_len[b] outside [1, Tx] sets *bad (int32, device; never cleared here) and is clamped. */
int ft_gen_durations(float* dur, const long* x_len, int B, int Tx, long* mel_len, int* bad, void* stream);
/* y[b,t,:] = x[b,tok(t),:] for t < total[b], else 0; optional src_idx[B,Tm] (token or -1). Bit-exact copy. */
int ft_lr_expand(const float* x, const int* cum, float* y, int* src_idx, int B, int Tx, int Tm, int C,
                 void* stream);
/* dx[b,j,:] = sum of dy rows of token j (fixed order) */
int ft_lr_bwd(const float* dy, const int* cum, float* dx, int B, int Tx, int Tm, int C, void* stream);
/* The same pair with the FRAME side time-major ([Tm,B,C]) -- the layout of the recurrences' buffers.  They carry the
 * decoder LSTM's input projection through the LengthRegulator: the projection is a row-wise linear map and the
 * regulator only repeats rows, so x_tok * W_ih^T + b_ih is formed once per TOKEN (4,096 rows at the benchmark shape
 * instead of 26,912 frames; same kernel, same k order: every row has the bits the frame-level GEMM gives it) and
 * ft_lr_expand_tm writes it out per frame; pad_row (C floats, optional) is what frames beyond an item's length hold
 * -- the projection of the regulator's zero rows is the bias.  Backward: ft_lr_bwd_tm sums d(pre-activations) over each
 * token's frames, and the input / weight gradients of W_ih are token-level GEMMs (forward_tacotron.py:145-152). */
int ft_lr_expand_tm(const float* x, const int* cum, const float* pad_row, float* y, int B, int Tx, int Tm, int C,
                    void* stream);
/* dtail (optional, [B,C]): per item, the sum of the frames beyond its last token (t >= total[b]) -- they reach no token,
 * but the bias gradients are column sums over ALL frames (an unpacked LSTM runs over those frames too) */
int ft_lr_bwd_tm(const float* dy, const int* cum, float* dx, float* dtail, int B, int Tx, int Tm, int C, void* stream);

/* ---- nn.BatchNorm1d of BatchNormConv (common_layers.py:51,57) on channels-last y[B,Tbuf,C] ----------- */
/* group > 0 = CBHG bank buffer [B,T+1,K*group]: channel c belongs to kernel size k=c/group+1 and has
 * Tbuf-1 valid rows for odd k, Tbuf for even k (common_layers.py:97-99); group = 0: all Tbuf rows valid.
 * train fwd: batch statistics (biased var) over valid rows -> save_mean/save_rstd; running stats updated
 * in place (momentum, unbiased var), *num_batches_tracked += 1; out[B,Tout,C] = bn(y)[:, :Tout] (+residual). */
size_t ft_bn_workspace(int B, int Tbuf, int C);
/* BatchNormConv with the statistics pass fused into the convolution (north_star: "BatchNormConv fused"): the conv's
 * GEMM epilogue reduces (sum, sum of squares) of its 128-row output tile per channel -- doubles, fixed order -- into
 * `partial` ([nchunks][C][2], ft_conv_stats_workspace bytes) while the tile is still in the MFMA accumulators, so the
 * activation is not read back for the statistics; launches that do not take the 128x128 kernel (token-side shapes) run
 * the stand-alone column pass instead -- either way *nchunks (HOST int) tells ft_bn_train_from_partials how many partial
 * rows to finalize (ordered sum; mean / biased var / running stats as ft_bn_train_fwd) before it normalises.
 * conv1d: y contiguous [B,Tout,Cout].  conv_bank: training-mode bank buffer [B,T+1,K*C]; odd-k members count T rows.
 * ft_conv1d_fwd_stats_workspace >= ft_conv_stats_workspace: it adds room for per-tap output slabs where a token-side
 * convolution (too few 128x128 tiles to fill the chip) runs its k taps as independent tasks followed by one ordered sum;
 * a caller that passes only ft_conv_stats_workspace bytes simply gets the single-task form. */
size_t ft_conv_stats_workspace(int B, int Tbuf, int C);
size_t ft_conv1d_fwd_stats_workspace(int B, int Tout, int Cout, int k);
int ft_conv1d_fwd_stats(const float* x, long ldx, const float* wp, float* y, long ldy, int B, int T, int Cin, int Cout,
                        int k, int Tout, int relu, double* partial, size_t partial_bytes, int* nchunks, void* stream);
int ft_conv_bank_fwd_stats(const float* x, long ldx, const float* wp_all, float* ybank, int B, int T, int Cin, int C,
                           int K, int relu, double* partial, size_t partial_bytes, int* nchunks, void* stream);
int ft_bn_train_from_partials(const double* partial, int nchunks, const float* y, const float* gamma, const float* beta,
                              const float* residual, float* out, float* running_mean, float* running_var,
                              long* num_batches_tracked, float* save_mean, float* save_rstd, int B, int Tbuf, int Tout,
                              int C, int group, float momentum, float eps, void* stream);
/* CBHG conv bank, training mode (common_layers.py:100-105): BatchNorm apply fused with MaxPool1d(2,1,1)[:Tout].
 * ft_bn_pool_from_partials: finalize the partials as ft_bn_train_from_partials, then out[B,Tout,C][t] =
 *   max(z[t-1], z[t]) with z = bn(y) recomputed on the fly -- z is never written.
 * ft_bn_pool_bwd: dout[B,Tout,C] is the gradient of the POOLED output; the BatchNorm output's gradient (torch's
 *   max_pool rule: a window's gradient goes to its first maximal element) is recomputed from y in both passes
 *   (statistics and apply), so neither z nor dz ever exists in memory.  dy / dgamma / dbeta as ft_bn_bwd.
 * Both need C % 4 == 0, group % 4 == 0 and 16-byte aligned buffers (FT_ERR otherwise: callers fall back to
 * ft_bn_train_from_partials + ft_maxpool2_fwd / ft_maxpool2_bwd + ft_bn_bwd). */
int ft_bn_pool_from_partials(const double* partial, int nchunks, const float* y, const float* gamma, const float* beta,
                             float* out, float* running_mean, float* running_var, long* num_batches_tracked,
                             float* save_mean, float* save_rstd, int B, int Tbuf, int Tout, int C, int group,
                             float momentum, float eps, void* stream);
int ft_bn_pool_bwd(const float* dout, const float* y, const float* gamma, const float* beta, const float* save_mean,
                   const float* save_rstd, float* dy, float* dgamma, float* dbeta, int B, int Tbuf, int Tout, int C,
                   int group, int relu, void* workspace, size_t workspace_bytes, void* stream);
int ft_bn_train_fwd(const float* y, const float* gamma, const float* beta, const float* residual, float* out,
                    float* running_mean, float* running_var, long* num_batches_tracked, float* save_mean,
                    float* save_rstd, int B, int Tbuf, int Tout, int C, int group, float momentum, float eps,
                    void* workspace, size_t workspace_bytes, void* stream);
/* dy[B,Tbuf,C] (0 on invalid rows), dgamma, dbeta from dout[B,Tout,C]; relu=1 also applies the ReLU mask
 * (y>0) of the conv->ReLU->BN order (common_layers.py:55-57) */
int ft_bn_bwd(const float* dout, const float* y, const float* gamma, const float* save_mean, const float* save_rstd,
              float* dy, float* dgamma, float* dbeta, int B, int Tbuf, int Tout, int C, int group, int relu,
              void* workspace, size_t workspace_bytes, void* stream);
/* eval mode: scale = gamma/sqrt(running_var+eps), shift = beta - running_mean*scale (fed to the conv epilogue) */
int ft_bn_fold_eval(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                    float eps, float* scale, float* shift, int C, void* stream);
/* out[c] (+)= scale * sum_rows x[row*ldx + c]   (bias gradients; ordered, reproducible) */
size_t ft_colsum_workspace(int rows, int C);
int ft_colsum(const float* x, long ldx, float* out, int rows, int C, float scale, int accumulate, void* workspace,
              size_t workspace_bytes, void* stream);
/* column sums of two matrices of one shape (x0 -> out0, x1 -> out1) in one partial + one finalize launch: LayerNorm's
 * dgamma = colsum(dy * xhat), dbeta = colsum(dy) */
int ft_colsum2(const float* x0, const float* x1, long ldx, float* out0, float* out1, int rows, int C, void* workspace,
               size_t workspace_bytes, void* stream);
/* n <= 16 column sums over matrices with the same row count in ONE partial + ONE finalize launch: out[i][c] = sum_r
 * x[i][r * ld[i] + c].  Every sum keeps the chunking and summation order of its own ft_colsum call (bit-identical). */
size_t ft_colsum_batch_workspace(int n, const int* C, int rows);
int ft_colsum_batch(int n, const float* const* x, const long* ld, float* const* out, const int* C, int rows,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- F.dropout (forward_tacotron.py:35 ; common_layers.py:106,110) and scalar scale (x/alpha, :39) ----- */
/* out = keep ? x/(1-p) : 0 with keep(i) = hash(seed,i) >= p; calling it on the gradient with the same seed
 * is the backward (no mask tensor).  torch's RNG stream cannot be matched: parity runs use p = 0, or rebuild the mask
 * on the host (tests/dropout_cpu.py).  hash = ft_hash32 (csrc/ft_common.h), keep(i) = (hash >> 8) * 2^-24 >= p.
 * SEED CONTRACT (every entry below that takes a dropout or draw seed): seeds of different sites must differ in the HIGH
 * 32-bit word, and not only in its top ten bits; two seeds with equal high words give one mask permuted by an XOR of
 * the index (seeds 1, 2, 3, ... are shuffles of one mask).  base._seed() and tacotron.dropout_seed() satisfy this. */
int ft_dropout(const float* x, float* out, long n, float p, uint64_t seed, void* stream);
int ft_scale(const float* x, float* out, long n, float s, void* stream);
/* n <= 64 independent device-to-device copies in ONE launch: dst[i][0:len[i]] = src[i][0:len[i]]  (src / dst / len are
 * HOST arrays).  Used to hand fused-kernel results (a conv bank's K dgamma / dbeta slices, an RNN's four bias
 * gradients) to their slots in the flat gradient buffer without one copy launch per parameter. */
int ft_copy_segments(const float* const* src, float* const* dst, const long* len, int n, void* stream);

/* ---- nn.Embedding (forward_tacotron.py:18,31,73,133) -------------------------------------------------- */
/* out[row,:] = w[idx[row],:] ; *err_flag set to 1 on an out-of-range index (row zero-filled) */
int ft_embedding_fwd(const long* idx, const float* w, float* out, long rows, int C, int V, int* err_flag,
                     void* stream);
/* The embedding of a RAGGED inference batch (ForwardTacotron.generate_batch; the reference's generate,
 * forward_tacotron.py:167-234, passes no lengths): idx [B,T], lens int64 [B] (device).  out[b,t,:] = w[idx[b,t],:] at
 * t < lens[b] and exactly 0 at t >= lens[b], where idx is NOT read: the padding may hold any id, also one outside
 * [0, V), and does not raise *err_flag. */
int ft_embedding_fwd_lens(const long* idx, const long* lens, const float* w, float* out, int B, int T, int C, int V,
                          int* err_flag, void* stream);
/* backward: onehot[rows,V] = (idx == v); dW[V,C] = onehot^T * dout via ft_linear_bwd_weight (ordered, reproducible) */
int ft_onehot(const long* idx, float* out, long rows, int V, void* stream);

/* ---- HighwayNetwork gate (common_layers.py:35-40); x12 = [W1 x + b1 | W2 x + b2] from ft_linear_multi_fwd */
int ft_highway_gate_fwd(const float* x12, const float* x, float* out, long rows, int C, void* stream);
/* d12 = gradient wrt x12, dx = direct-path gradient dout*(1-g) (caller adds d12*[W1;W2]) */
int ft_highway_gate_bwd(const float* dout, const float* x12, const float* x, float* d12, float* dx, long rows, int C,
                        void* stream);

/* The same layer with the gate INSIDE the GEMMs (C % 32 == 0; the two calls above stay for other widths).
 * ft_highway_pack: w12i [2C, C] = the 32-row interleave of W1 and W2 (row n: unit (n/64)*32 + n%32 of W1 if n%64 < 32, else
 *   of W2), so that one accumulator lane pair holds W1 x and W2 x of the same unit.
 * ft_highway_fwd: out [rows, C] = g * relu(y1) + (1 - g) * x with y1 | y2 = x W1^T + b1 | x W2^T + b2, g = sigmoid(y2), from
 *   the epilogue of ONE product x * w12i^T; x12 (may be NULL) receives y1 | y2 as [rows, 2C] for the backward.
 * ft_highway_bwd_data: dx [rows, C] += d12[:, :C] W1 + d12[:, C:] W2 (dx holds the direct-path term; w1 / w2 are W^T
 *   [C, C] if w_transposed).  With below_* set, dx is d(out) of the highway layer BELOW and the epilogue turns it into that
 *   layer's ft_highway_gate_bwd outputs at once: below_d12 [rows, 2C] and dx = direct-path term of the layer below
 *   (below_x12 / below_x = that layer's saved pre-activations and input). */
int ft_highway_pack(const float* w1, const float* w2, float* w12i, int C, void* stream);
int ft_highway_fwd(const float* x, const float* w12i, const float* b1, const float* b2, float* out, float* x12, int rows,
                   int C, void* stream);
int ft_highway_bwd_data(const float* d12, const float* w1, const float* w2, int w_transposed, float* dx, int rows, int C,
                        const float* below_x12, const float* below_x, float* below_d12, void* stream);

/* ---- MaxPool1d(kernel 2, stride 1, padding 1)[:T] (common_layers.py:78,105): out[t]=max(x[t-1],x[t]) ---- */
int ft_maxpool2_fwd(const float* x, float* out, int B, int T, int C, void* stream);
/* with per-item lengths (ragged inference batch): out[b,t] = 0 at t >= lens[b] -- row lens[b] of the plain form holds
 * x[lens[b]-1], which CBHG.conv_project1 (common_layers.py:107) would read from row lens[b]-1 */
int ft_maxpool2_fwd_lens(const float* x, const long* lens, float* out, int B, int T, int C, void* stream);
int ft_maxpool2_bwd(const float* dout, const float* x, float* dx, int B, int T, int C, void* stream);

/* ---- pitch/energy conditioning (forward_tacotron.py:111-112,137-143): Conv1d(1->C,k3,p1)+bias, scaled add */
int ft_cond_add_fwd(const float* x, const float* pitch, const float* energy, const float* w_pitch,
                    const float* b_pitch, const float* w_energy, const float* b_energy, float pitch_strength,
                    float energy_strength, float* out, int B, int T, int C, int x_time_major, void* stream);
/* taps[row][8] = [p[t-1],p[t],p[t+1],1,e[t-1],e[t],e[t+1],1]; weight/bias grads = dy^T taps (ft_linear_bwd_weight) */
int ft_cond_taps(const float* pitch, const float* energy, float* taps, int B, int T, void* stream);

/* ---- multispeaker plumbing (models/multi_forward_tacotron.py:39-42,83-85,208-210) ---------------------- */
/* out[b,t,:] = [ a[b,t,:Ca] | b2[b,t,:Cb] | semb[b,:S] ]  (speaker embedding broadcast over t); a may be a
 * time-major [T,B,Ca] recurrence output; b2 / semb optional (Cb = 0 / S = 0) */
int ft_concat_cols(const float* a, int Ca, const float* b2, int Cb, const float* semb, int S, float* out, int B,
                   int T, int a_time_major, void* stream);
/* dst[b,t,:C] = src[(b,t)*ld + col0 + :C] ; dst optionally time-major (backward of the concat) */
int ft_slice_cols(const float* src, long ld, int col0, int C, float* dst, int B, int T, int dst_time_major,
                  void* stream);
/* nn.CrossEntropyLoss(ignore_index) on logits[rows,K] / int64 target[rows] (trainer/multi_forward_trainer.py:34,88) */
size_t ft_cross_entropy_workspace(void);
int ft_cross_entropy_fwd(const float* logits, const long* target, long rows, int K, long ignore_index, float* loss,
                         float* inv_count, void* workspace, size_t workspace_bytes, void* stream);
int ft_cross_entropy_bwd(const float* logits, const long* target, const float* inv_count, const float* grad_out,
                         float* dlogits, long rows, int K, long ignore_index, void* stream);

/* ---- output layout + ForwardTacotron._pad (forward_tacotron.py:155,159,161-162,236-239) ---------------- */
/* out[b,c,t] = t < T ? x[b,t,c] : pad, t < Tout   ([B,T,C] -> [B,C,Tout]) ; bwd is the masked transpose back */
int ft_transpose_pad_fwd(const float* x, float* out, int B, int T, int C, int Tout, float pad, void* stream);
/* per-item lengths (ragged inference batch): out[b,c,t] = t < min(lens[b], T) ? x[b,t,c] : pad, t < Tout */
int ft_transpose_pad_lens_fwd(const float* x, const long* lens, float* out, int B, int T, int C, int Tout, float pad,
                              void* stream);
int ft_transpose_pad_bwd(const float* dout, float* dx, int B, int T, int C, int Tout, void* stream);

/* ---- MaskedL1 (trainer/common.py:69-92) on [B,C,T] with int64 lens ----------------------------------- */
size_t ft_masked_l1_workspace(void);
int ft_masked_l1_fwd(const float* x, const float* target, const long* lens, float* loss, float* inv_denom, int B,
                     int C, int T, void* workspace, size_t workspace_bytes, void* stream);
/* dx = sign(x-target)*mask*inv_denom * factor * (grad_out ? grad_out[0] : 1) */
int ft_masked_l1_bwd(const float* x, const float* target, const long* lens, const float* inv_denom,
                     const float* grad_out, float factor, float* dx, int B, int C, int T, void* stream);

/* ---- nn.GRU(bidirectional, batch_first), h0 = 0 (common_layers.py:89,123 ; forward_tacotron.py:24,37) - */
/* ALL recurrence buffers are TIME-major: xp[T,B,2*3H] = x W_ih^T + b_ih (dir 0 | dir 1); out[T,B,2H];
 * gates[T,B,2,4H] = (r,z,n,W_hn h+b_hn) or NULL */
/* `workspace` (ft_rnn_workspace(gates,B,H) bytes, may be NULL) enables the PERSISTENT form: one launch runs all T
 * steps with W_hh resident in registers and h exchanged between workgroups inside the kernel (bounded spins).
 * It is used when H % 16 == 0, the grid is co-resident per the occupancy query and FT_RNN_PERSISTENT != 0;
 * otherwise one kernel per timestep is launched.  A launch is admitted only while the persistent grids still in flight
 * on OTHER streams of the device plus its own fit every XCD in the worst case, because every workgroup spins until its
 * whole grid is resident.  Grids whose (direction, batch group) groups each fit one XCD slot are laid out that way and
 * hand h / d(gates) over through that XCD's L2 (placement verified in the kernel, agent-scope protocol otherwise).
 * Faults: a workgroup whose bounded poll runs out sets the device's STICKY fault word and leaves (the grid drains);
 * no launch clears that word.  ft_clip_grad_norm / ft_adam_step read it on the device and skip the parameter update;
 * ft_rnn_status(clear) synchronises the device, returns an error if the word is set and (clear != 0) resets it. */
size_t ft_rnn_workspace(int gates, int B, int H);
int ft_rnn_status(int clear);
/* runtime override of FT_RNN_PERSISTENT (1 = allow the persistent form); returns the previous setting */
int ft_rnn_set_persistent(int enabled);
/* bound of the arrival polls (0 restores the default 2^18; -1 = fault injection for tests: every poll of every
 * later launch fails at once, deterministically); returns the previous bound (0 while injecting) */
int ft_rnn_set_max_spins(int max_spins);
/* Tell the admission bookkeeping that `waiting_stream` has just been made to wait for everything enqueued so far on
 * `joined_stream` (hipStreamWaitEvent / torch's wait_stream): the joined stream's earlier persistent launches then
 * precede whatever the waiting stream launches next and no longer count against it.  Optional -- without it the
 * bookkeeping is merely conservative. */
int ft_rnn_note_join(void* waiting_stream, void* joined_stream);
/* A HIP stream restricted to the first `cus_per_xcd` CUs of every XCD (hipExtStreamCreateWithCUMask).  New work, no
 * reference counterpart (the reference is single-stream, trainer/forward_trainer.py:69-99): trainer.TrainStep puts its
 * weight-gradient side stream on one, so that the one-wave weight-gradient GEMMs leave a few CUs per XCD to the small
 * dependent kernels of the step's critical stream.  ft_stream_destroy releases it. */
int ft_stream_create_cu_limited(int cus_per_xcd, void** stream);
int ft_stream_destroy(void* stream);
/* (direction, batch group) groups of persistent launches that ran the XCD-local hand-off / the agent-scope one since
 * the library loaded (synchronises the device) */
int ft_rnn_mode_counts(long* xcd_local_groups, long* agent_scope_groups);
/* launches that ran in the persistent form / that did not fit the chip even alone (and ran per-step) since the library
 * loaded; ft_rnn_waited_launches: persistent launches whose stream was first made to wait for other streams' */
int ft_rnn_counters(long* persistent_launches, long* refused_launches);
/* Share (percent) of ONE XCD's CUs the persistent recurrence of this shape holds while it runs (gates 3 = GRU, 4 = LSTM;
 * backward != 0: the BPTT kernel); -1: it would not run persistent.  Two persistent launches on different streams are
 * co-resident while their shares add up to at most ft_rnn_admit_budget_pct(); a launch at 100 fills whole XCDs, and no
 * other kernel is dispatched anywhere while it is resident (the dispatcher deals workgroups to the XCDs round-robin and
 * waits at the first full one). */
int ft_rnn_xcd_fill_pct(int gates, int backward, int B, int T, int H);
int ft_rnn_admit_budget_pct(void);
/* The persistent form a recurrence of this shape would take under the current FT_RNN_* environment (gates 3 = GRU,
 * 4 = LSTM; backward != 0: the BPTT, always both directions; nd = 1 | 2 directions of the forward), decided on the host
 * alone: no device is touched, nothing is launched, aligned buffers and a workspace of ft_rnn_workspace bytes are
 * assumed.  form[FT_RNN_PLAN_FIELDS] receives, in this order:
 *   kind (0 = per-step kernels, and every other field 0; 1 = forward, 2 = all-gather BPTT, 3 = reduce-scatter BPTT),
 *   the six template arguments of the kernel as the FT_RNN_DEBUG line prints them (unused ones -1),
 *   threads per workgroup, batch rows per workgroup, workgroups per (direction, batch group) group (nchunks), groups,
 *   workgroups in all, workgroups per XCD slot in the aligned layout and in the spread one (0: the layout does not
 *   apply), 1 if the kernel hands over by granules inside an XCD, workspace bytes the form needs.
 * Whether a launch is then admitted depends on the kernel's occupancy and on what is in flight (ft_rnn_xcd_fill_pct). */
#define FT_RNN_PLAN_FIELDS 16
int ft_rnn_plan(int gates, int backward, int B, int T, int H, int nd, long* form);
int ft_rnn_waited_launches(void);
int ft_gru_fwd(const float* xp, const float* whh_f, const float* whh_r, const float* bhh_f, const float* bhh_r,
               float* out, float* gates, int B, int T, int H, void* workspace, size_t workspace_bytes,
               void* stream);
/* pack_padded_sequence -> nn.GRU -> pad_packed_sequence (common_layers.py:89,123 over a ragged inference batch; the
 * semantics of ft_lstm_fwd): item b runs over lens[b] (int64 [B], device) steps in both directions, the reverse one
 * from t = lens[b] - 1; out is ZERO at t >= lens[b]. */
int ft_gru_fwd_lens(const float* xp, const float* whh_f, const float* whh_r, const float* bhh_f, const float* bhh_r,
                    const long* lens, float* out, float* gates, int B, int T, int H, void* workspace,
                    size_t workspace_bytes, void* stream);
/* BPTT: dout[T,B,2H]; whhT = W_hh^T [H,3H]; dxp / dhp [T,B,2*3H] = d(pre-activations) wrt input / hidden
 * projections; carry [B,2,H] scratch.  Weight grads follow from ft_linear_bwd_weight on dxp / dhp. */
int ft_gru_bwd(const float* dout, const float* out, const float* gates, const float* whhT_f, const float* whhT_r,
               float* dxp, float* dhp, float* carry, int B, int T, int H, void* workspace, size_t workspace_bytes,
               void* stream);

/* ---- pack_padded_sequence -> nn.LSTM(bidirectional) -> pad_packed_sequence (forward_tacotron.py:96-99,147-152)
 * lens (int64 [B], device) or NULL = run over the padded length (generate path, :224).  Item b is processed
 * over exactly lens[b] frames in both directions; out_raw / cstate [T,B,2H] (time-major, like xp / gates /
 * dgates) are ZERO at t >= lens[b]; ft_fill_padded converts to batch-major [B,T,2H] and writes the
 * padding_value the reference's unpack inserts (lens NULL: plain layout change). xp includes b_ih; b_hh added here. */
int ft_lstm_fwd(const float* xp, const float* whh_f, const float* whh_r, const float* bhh_f, const float* bhh_r,
                const long* lens, float* out_raw, float* cstate, float* gates, int B, int T, int H,
                void* workspace, size_t workspace_bytes, void* stream);
int ft_lstm_bwd(const float* dout, const float* out_raw, const float* cstate, const float* gates,
                const float* whhT_f, const float* whhT_r, const long* lens, float* dgates, float* carry, int B, int T,
                int H, void* workspace, size_t workspace_bytes, void* stream);
/* One direction (models/tacotron.py Decoder.res_rnn1 / res_rnn2 under teacher forcing: nn.LSTMCell over T steps from
 * zero states): xp [T,B,4H] (x W_ih^T + b_ih, time-major), out_raw / cstate [T,B,H]; b_hh added here.  Same kernels as
 * ft_lstm_fwd with the direction count 1: the persistent form where it fits (workspace: ft_rnn_workspace(4, B, H)),
 * the per-step kernels otherwise. */
int ft_lstm_fwd_uni(const float* xp, const float* whh, const float* bhh, float* out_raw, float* cstate, int B, int T,
                    int H, void* workspace, size_t workspace_bytes, void* stream);
/* ---- a recurrent LAYER's forward with the input projection overlapped with the recurrence (no reference counterpart:
 * nn.LSTM / nn.GRU, forward_tacotron.py:96-99,147-152 / common_layers.py:89,123, run the projection in front).
 * x [B,T,in_f] batch-major; xp [T,B,2*G*H] (scratch for the projection, G = 4 | 3); the other arguments as in
 * ft_lstm_fwd / ft_gru_fwd.  x * W_ih^T + b_ih is formed in `nchunks` time chunks: chunk 0 of both directions on
 * `stream`, the others on `side_stream`, each followed by a one-thread kernel that raises gate[direction]; the
 * persistent recurrence is launched right behind chunk 0 and polls (bounded) the gate word before it reads a row of a
 * chunk it has not seen complete.  gate: >= 2 device words owned by the call.  rev_lead: chunks of the reverse direction
 * issued first (a packed item of length L starts at t = L - 1).  nchunks < 2 / side_stream NULL or == stream: the
 * projection runs whole, in front.  If the persistent form is refused, `stream` first waits for all chunks.  Results are
 * bit-identical to ft_linear_multi_fwd + ft_lstm_fwd / ft_gru_fwd. */
int ft_lstm_layer_fwd(const float* x, int in_f, const float* wih_f, const float* wih_r, const float* bih_f,
                      const float* bih_r, float* xp, const float* whh_f, const float* whh_r, const float* bhh_f,
                      const float* bhh_r, const long* lens, float* out_raw, float* cstate, float* gates, int B, int T,
                      int H, void* workspace, size_t workspace_bytes, unsigned* gate, int nchunks, int rev_lead,
                      void* stream, void* side_stream);
int ft_gru_layer_fwd(const float* x, int in_f, const float* wih_f, const float* wih_r, const float* bih_f,
                     const float* bih_r, float* xp, const float* whh_f, const float* whh_r, const float* bhh_f,
                     const float* bhh_r, float* out, float* gates, int B, int T, int H, void* workspace,
                     size_t workspace_bytes, unsigned* gate, int nchunks, void* stream, void* side_stream);
/* ft_gru_layer_fwd over a packed batch (ft_gru_fwd_lens); rev_lead as in ft_lstm_layer_fwd */
int ft_gru_layer_fwd_lens(const float* x, int in_f, const float* wih_f, const float* wih_r, const float* bih_f,
                          const float* bih_r, float* xp, const float* whh_f, const float* whh_r, const float* bhh_f,
                          const float* bhh_r, const long* lens, float* out, float* gates, int B, int T, int H,
                          void* workspace, size_t workspace_bytes, unsigned* gate, int nchunks, int rev_lead,
                          void* stream, void* side_stream);
int ft_fill_padded(const float* raw, const long* lens, float* out, int B, int T, int C, float pad, void* stream);
int ft_mask_rows(const float* src, const long* lens, float* dst, int B, int T, int C, void* stream);
/* [B,T,C] -> [T,B,C] (dst_time_major = 1) or back (0) */
int ft_bt_transpose(const float* src, float* dst, int B, int T, int C, int dst_time_major, void* stream);

/* ---- clip_grad_norm_ + torch.optim.Adam (trainer/forward_trainer.py:95-99 ; train_forward.py:76) ------ */
/* over FLAT fp32 buffers (all parameters back to back, 16-B aligned).  coef_and_norm holds FOUR floats:
 * [0] = pre_scale * min(1, max_norm/(norm+1e-6)), [1] = norm = pre_scale*||grads||_2 (pre_scale = 1/world_size when
 * the buffer holds an all-reduced SUM), [2] = 1 if the device's recurrence-fault word is set, 2 if only fault_lane says
 * so (then [0] = 0, [1] = NaN and ft_adam_step leaves params / moments untouched), [3] = 0; max_norm <= 0 disables
 * clipping.  Stays on device: no host sync.
 * Data parallelism (new work: the reference is single device, train_forward.py:70): a recurrence fault must be GLOBAL --
 * the faulting rank's garbage gradient is summed into every rank's buckets.  ft_fault_lane_set writes this device's fault
 * word as 1.0 / 0.0 into lane[0] (lane = 4 floats, 16-B aligned; [1..3] = 0); the caller SUM-all-reduces the lane with the
 * gradient and hands it to ft_clip_grad_norm as fault_lane (NULL: single device): a non-zero lane[0] skips the update on
 * every rank alike. */
size_t ft_grad_norm_workspace(void);
int ft_clip_grad_norm(const float* grads, long n, float max_norm, float pre_scale, const float* fault_lane,
                      float* coef_and_norm, void* workspace, size_t workspace_bytes, void* stream);
int ft_fault_lane_set(float* lane, void* stream);
/* dst[0..nwords) <- snapshot (4-byte words) iff coef[2] != 0 (ft_clip_grad_norm's record): puts the buffers a forward
 * pass updates in place (BatchNorm running_mean / running_var / num_batches_tracked, forward_tacotron.py:101,126-127
 * `step`) back to their values from before a faulted step; a no-op launch otherwise */
int ft_guarded_restore(void* dst, const void* snapshot, long nwords, const float* coef, void* stream);
/* Adam, torch defaults semantics (no weight decay / amsgrad): g = grads*coef[0]; step counts from 1; coef (may be NULL)
 * is ft_clip_grad_norm's 4-float record: a set [2] skips the update */
int ft_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                 float beta2, float eps, long step, const float* coef, void* stream);

/* ---- fused self-attention, bf16 matmul mode (nn.MultiheadAttention inside FFTBlock, common_layers.py:172-174) ---- */
/* qkv [B,T,3d] = the in-projection's output rows (q | k | v, d = nheads*hd, head h at columns h*hd of each third), fp32;
 * key_pad [B,T] bytes (non-zero = padded key) or NULL.  ft_attn_fwd: att [B,T,d] = concat_h softmax(scale q_h k_h^T +
 * mask) v_h with attention dropout p_drop (the counter-based mask of ft_softmax_fwd: element index = flat index into
 * [B,nheads,T,T], same seed -> same mask), and lse2 [B,nheads,T] = log2-domain log-sum-exp per query row for the
 * backward.  One flash-style launch: the [B,nheads,T,T] scores never reach memory.  Operands are rounded to bf16 while
 * staged (bf16 MFMA, fp32 statistics / accumulation / outputs): this IS the bf16 mode, there is no fp32-exact variant (the
 * fp32 mode keeps ft_bgemm_* + ft_softmax_*).  hd = 64 or 128.
 * ft_attn_bwd: dqkv [B,T,3d] (every element written) from datt = d(att); recomputes the probabilities from qkv and lse2
 * (three launches: row sums of datt*att, dQ, dK+dV; no atomics, bitwise reproducible).  workspace: ft_attn_workspace.
 * seed: under ft_dropout's seed contract (distinct high words between sites; equal high words = XOR-permuted masks). */
size_t ft_attn_workspace(int B, int T, int nheads);
int ft_attn_fwd(const float* qkv, const unsigned char* key_pad, float* att, float* lse2, int B, int T, int nheads, int hd,
                float scale, float p_drop, uint64_t seed, void* stream);
int ft_attn_bwd(const float* qkv, const float* att, const float* datt, const unsigned char* key_pad, const float* lse2,
                float* dqkv, int B, int T, int nheads, int hd, float scale, float p_drop, uint64_t seed, void* workspace,
                size_t workspace_bytes, void* stream);

/* ---- length-aware fused self-attention, inference, both matmul modes (FastPitch.generate_batch) ------------------- */
/* qkv [B,T,3d] as ft_attn_fwd; lens int64 [B] on the device.  For item b, L = min(max(lens[b], 0), T): rows t < L of att
 * [B,T,d] hold softmax(scale q_h k_h^T over the keys < L) v_h, rows t >= L hold exactly 0.  No dropout, no log-sum-exp, no
 * byte mask.  qkv rows at t >= L are never read into arithmetic (they may hold NaN); workgroups whose queries all lie past
 * L store zeros and leave, every other key loop ends at ceil(L / 64) blocks.  bf16 = 1: ft_attn_fwd's arithmetic (valid
 * rows bit-equal to it with the byte mask t >= L at p_drop = 0); bf16 = 0: fp32-exact products (v_mfma_f32_32x32x2_f32).
 * hd = 64, 128, 192 or 256; qkv and att 16-byte aligned.  192 / 256 (the multispeaker models' 384- and 512-wide stacks on
 * 2 heads) run in 32-key blocks with the head width split over a pair of waves (csrc/ft_attn_lens.hip): same contract,
 * key loops end at ceil(L / 32) blocks, workgroups of 64 queries; no byte-mask twin, hence no bit-equality claim. */
int ft_attn_fwd_lens(const float* qkv, const int64_t* lens, float* att, int B, int T, int nheads, int hd, float scale,
                     int bf16, void* stream);
/* y [B,T,D] = LayerNorm(x + res) (res may be NULL) at t < lens[b], exactly 0 at t >= lens[b], where x / res are not read:
 * the inference add + LayerNorm in front of an FFTBlock's k > 1 convolutions on a ragged batch */
int ft_add_layernorm_fwd_lens(const float* x, const float* res, const float* gamma, const float* beta, const long* lens,
                              float* y, int B, int T, int D, float eps, void* stream);
/* ft_conv1d_bias_fwd whose epilogue stores zeros at t >= lens[b]; x must be zero there */
int ft_conv1d_bias_fwd_lens(const float* x, long ldx, const float* wp, const float* bias, float* y, long ldy,
                            const long* lens, int B, int T, int Cin, int Cout, int k, int relu, void* stream);
/* flag[0] |= 2 if idx [B,T] holds the pad id 0 at some t < lens[b] (ids at t >= lens[b] are not read) */
int ft_check_tokens_lens(const long* idx, const long* lens, int B, int T, int* flag, void* stream);

/* ---- the multispeaker models on a ragged batch (MultiForwardTacotron / MultiFastPitch.generate_batch) ------------- */
/* The front of a speaker-conditioned predictor (and of MultiFastPitch's trunk), ft_embedding_fwd (+ a second one) +
 * ft_concat_cols in one launch: out[b,t,:] = [ emb[idx[b,t],:Ce] | cond_emb[cond[b,t],:Cc] | semb[b,:S] ] at
 * t < lens[b] and exactly 0 at t >= lens[b], where idx and cond are NOT read (any id there, also one out of range, is
 * harmless and does not raise *err_flag).  idx, cond [B,T] int64, lens int64 [B] on the device, semb [B,S]: one speaker
 * row per item.  The cond part and the speaker part are optional (Cc = 0 / S = 0, their pointers may then be NULL). */
int ft_predictor_front_lens(const long* idx, const long* cond, const long* lens, const float* emb, int Ce, int V,
                            const float* cond_emb, int Cc, int Vc, const float* semb, int S, float* out, int B, int T,
                            int* err_flag, void* stream);
/* out[b,t] (int64) = the index of the first maximum of logits[b,t,:K] at t < lens[b], 0 at t >= lens[b] (logits are not
 * read there).  torch.argmax's semantics: the first index on ties, a NaN counts as the maximum. */
int ft_argmax_lens(const float* logits, const long* lens, long* out, int B, int T, int K, void* stream);

/* ---- a whole FFTBlock per call (common_layers.py:148-185), bf16 matmul mode with the fused attention ------------ */
/* The FastPitch step is ~900 launches for ~13 ms of GPU work: issued one entry point at a time from Python it is bound by
 * the host (15 us per launch).  These two calls issue every launch of n consecutive FFTBlocks -- forward: in-projection,
 * ft_attn_fwd, out-projection, add + LayerNorm, conv1 + ReLU, conv2, add + LayerNorm; backward: the reverse, with the
 * two residual joins as accumulate epilogues, then the blocks' weight / bias / LayerNorm gradients on wgrad_stream behind
 * one event -- from C.  All buffers are the caller's; rows = B*T, row-major.  Same kernels, same order, same results as
 * the single entry points above. */
typedef struct FtFFTBlock {
  int B, T, d, nheads, dfft, k1, k2;
  float p_drop, eps1, eps2;
  uint64_t seed_attn, seed_ln1, seed_ln2;          /* three sites: ft_dropout's seed contract (distinct HIGH words) */
  const unsigned char* key_pad;                  /* [B,T] or NULL */
  /* parameters: torch layouts, the convolutions as tap-major packs [k][Cout][Cin] */
  const float *in_w, *in_b, *out_w, *out_b, *c1_wp, *c1_b, *c2_wp, *c2_b, *n1_g, *n1_b, *n2_g, *n2_b;
  /* backward only: W^T of the two projections and the transposed packs [k][Cin][Cout] (data gradients in the NT form) */
  const float *in_wT, *out_wT, *c1_wpt, *c2_wpt;
  /* activations: x [rows,d] in; the forward writes the rest, the backward reads them */
  const float* x;
  float *qkv, *att, *lse2, *sa, *s1, *mean1, *rstd1, *y1, *h1, *h2, *s2, *mean2, *rstd2, *y2;
} FtFFTBlock;
typedef struct FtFFTBlockGrads {
  const float* dy2;                              /* d(y2) [rows,d] */
  float* dx;                                     /* out: d(x) [rows,d] */
  /* scratch, kept by the caller until wgrad_stream has been joined: [rows,d] each except d_h1 / g_h1 [rows,dfft] and
   * dqkv [rows,3d] */
  float *t2, *d_y1, *d_h2, *d_h1, *g_h1, *t1, *d_h, *d_sa, *datt, *dqkv;
  /* parameter gradients, overwritten (torch layouts) */
  float *g_in_w, *g_in_b, *g_out_w, *g_out_b, *g_c1_w, *g_c1_b, *g_c2_w, *g_c2_b, *g_n1_g, *g_n1_b, *g_n2_g, *g_n2_b;
} FtFFTBlockGrads;
int ft_fft_blocks_fwd(const FtFFTBlock* blocks, int n, void* stream);
/* workspace: >= ft_attn_workspace(B,T,nheads) bytes (main stream); wgrad_workspace: >= ft_fft_block_wgrad_workspace(...)
 * bytes, used on wgrad_stream only (the four weight-gradient GEMMs of a block); sums_workspace: >=
 * ft_fft_block_sums_workspace(...) bytes, used on sums_stream only (its bias / LayerNorm column sums).  wgrad_stream /
 * sums_stream NULL = stream / wgrad_stream; sums_workspace NULL = the sums share wgrad_stream and its workspace, which
 * ft_fft_block_wgrad_workspace sizes for both (the larger of the two needs).  All three sizes are checked on entry. */
size_t ft_fft_block_wgrad_workspace(int B, int T, int d, int dfft, int k1, int k2);
size_t ft_fft_block_sums_workspace(int B, int T, int d, int dfft);
int ft_fft_blocks_bwd(const FtFFTBlock* blocks, const FtFFTBlockGrads* grads, int n, void* workspace,
                      size_t workspace_bytes, void* wgrad_workspace, size_t wgrad_workspace_bytes, void* sums_workspace,
                      size_t sums_workspace_bytes, void* stream, void* wgrad_stream, void* sums_stream);

/* ---- mel inversion + Griffin-Lim (utils/dsp.py:80-94 DSP.griffinlim ; gen_forward.py:109-116) ------------ */
/* The DFTs are GEMMs on ft_linear_fwd (frames read in place out of the zero-padded signal with ldx = hop); these are
 * the element-wise / gather pieces.  Complex spectra are split [N][2*Fp] = Re | Im, Fp = F rounded up to 4.
 * exp_transpose: log-mel [C,T] -> exp -> [T,C].  nnls_step: x = max(0, x - inv_l*g).  sub: out = a - b.
 * gl_init: proj = S * exp(2 pi i u) (u in [0,1), drawn by the host).  gl_phase: c = rebuilt - alpha*tprev (if has_prev);
 * proj = S * c / (|c| + FLT_MIN); tprev = rebuilt.  overlap_add: ypad [n_fft + hop*(N-1)] = sum of the (already windowed)
 * frames [N,n_fft] at offsets n*hop, times inv_wss (1 / summed squared window, 0 where that is below FLT_MIN), zero in
 * the n_fft/2 margins -- the signal sits at ypad + n_fft/2 and the padded buffer is the next STFT's operand. */
int ft_exp_transpose(const float* mel_log, float* out, int C, int T, void* stream);
int ft_nnls_step(float* x, const float* g, float inv_l, long n, void* stream);
int ft_sub(const float* a, const float* b, float* out, long n, void* stream);
int ft_gl_init(const float* u, const float* S, float* proj, int N, int Fp, void* stream);
int ft_gl_phase(const float* rebuilt, float* tprev, const float* S, float* proj, int N, int Fp, float alpha,
                int has_prev, void* stream);
int ft_overlap_add(const float* frames, const float* inv_wss, float* ypad, int N, int n_fft, int hop, void* stream);
/* The same for a RAGGED BATCH, one launch per call for all items (vocoder.GriffinLim.griffinlim_batch).  Item b has N_b =
 * mel_len[b] frames (int64 [B] on the device, read there) and owns rows [b*Tcap, (b+1)*Tcap) of every frame-major buffer
 * and samples [b*Tcap*hop, (b+1)*Tcap*hop) of the packed signal [B*Tcap*hop + n_fft]; Tcap*hop >= n_fft + hop*(Tmax-1), so
 * its padded signal fits, and all frames of all items are the rows of ONE GEMM with ldx = hop (rows n >= N_b of that
 * GEMM read the item's tail and its neighbour's head: garbage that gl_phase_ragged discards).  What an item gets depends
 * on its own data, N_b and (seed, n, m) alone -- not on B, Tcap, Tmax or its position -- and every mask is a select, so a
 * NaN elsewhere never reaches it.  A length outside [1, Tmax] is clamped into it (nothing indexes out of bounds) and sets
 * *err_flag = 1 (int32 on the device, zeroed by the caller; NULL = no report) in the two entries that take one.  All
 * buffers 16-byte aligned; Fp % 4 == 0, n_fft % 8 == 0, hop % 4 == 0: the accesses are 16 bytes wide.
 * gl_exp_transpose_ragged: mel [B,C,Tmax] -> out [B*Tcap, C] = exp(mel[b,c,n]) for n < N_b, 0 otherwise (mel is not read
 *   at n >= N_b).  gl_relu: x = max(x, 0) in place (the clip of the least-squares start; the forced-tile GEMM entry
 *   ft_linear_multi_fwd_as has no ReLU flag).
 * gl_init_ragged: proj [B*Tcap, 2Fp] = S * exp(2 pi i u) for n < N_b, zero rows otherwise; u = the given u [B*Tcap, Fp],
 *   or with u == NULL the counter-based draw u(seed, n, m) = (ft_hash32(seed, n*Fp + m) >> 8) * 2^-24 in [0, 1), where
 *   ft_hash32 is the library's 32-bit mixer of (seed, index) (csrc/ft_common.h; three multiply-xorshift rounds, the
 *   dropout generator): keyed on the frame n and bin m, NOT on b.  u_out (optional) [B*Tcap, Fp] receives the u used,
 *   0 at n >= N_b.  seed: under ft_dropout's seed contract -- draws meant to be independent need seeds that differ in
 *   the high word (not only in its top ten bits); seeds with equal high words, such as 1 and 2, give the SAME phases
 *   permuted by an XOR of the index n*Fp + m.
 * gl_phase_ragged: gl_phase on rows n < N_b; proj = 0 and tprev = 0 on the others, whatever `rebuilt` holds there.
 * overlap_add_ragged: ypad_b[t] = (sum over the item's own frames n < N_b, ascending, of frames[b*Tcap + n][t - n*hop]) /
 *   wss_{N_b}[t] for t in [n_fft/2, n_fft/2 + hop*(N_b-1)), 0 in the rest of the item's stride and in the n_fft tail
 *   behind the last item.  wss is accumulated beside the frames from w2 [n_fft] = the squared window in fp32 (same
 *   frames, same order; the quotient is acc * (1.0f / wss), and acc itself where wss <= FLT_MIN), so it holds for every
 *   N_b, including N_b < n_fft/hop where head and tail overlap.  Exactly one of ypad / wav is non-NULL: with wav
 *   [B, hop*(Tmax-1)] the same sums are written as the signal itself, wav[b][j] = ypad_b[n_fft/2 + j] for j <
 *   hop*(N_b-1), 0 beyond. */
int ft_gl_exp_transpose_ragged(const float* mel, const long* mel_len, float* out, int B, int C, int Tmax, int Tcap,
                               int* err_flag, void* stream);
int ft_gl_relu(float* x, long n, void* stream);
int ft_gl_init_ragged(const float* u, uint64_t seed, const float* S, const long* mel_len, float* proj, float* u_out,
                      int B, int Tcap, int Tmax, int Fp, int* err_flag, void* stream);
int ft_gl_phase_ragged(const float* rebuilt, float* tprev, const float* S, const long* mel_len, float* proj, int B,
                       int Tcap, int Tmax, int Fp, float alpha, int has_prev, void* stream);
int ft_overlap_add_ragged(const float* frames, const float* w2, const long* mel_len, float* ypad, float* wav, int B,
                          int Tcap, int Tmax, int n_fft, int hop, void* stream);

/* ---- audio front end: trim, peak-normalise, wav -> mel (utils/dsp.py:62-78,96-104 DSP.wav_to_mel / normalize /
 *      trim_silence ; preprocess.py:78-89, the audio half of Preprocessor._convert_file) ------------------------- */
/* A ragged batch is wav [B, ld] fp32 (16-byte aligned rows, ld % 4 == 0) with len [B] int64 on the device (item b is
 * wav[b, :len[b]], len <= Lmax <= ld; Lmax is the host's bound on the lengths and sizes every launch).
 * wav_trim_peak (two launches): frame mean squares of 2048-sample frames every 512 samples, centred, zero padding,
 * 1 + len / 512 frames; db = 10 log10(max(1e-10, ms)) - 10 log10(max(1e-10, max ms)); with do_trim, trim_start = 512 *
 * (first frame with db > -top_db), trim_end = min(len, 512 * (last such frame + 1)), (0, 0) if there is none (an all-zero
 * item is kept whole); without, (0, len).  wav_len = end - start, mel_len = 1 + wav_len / hop (0 for an empty item),
 * peak = max |y| over [start, end), scaled = peak_norm > 0 || (peak_norm == 0 && peak > 1) (peak_norm < 0: never).
 * An item's results depend on that item alone.
 * ws: ft_wav_trim_peak_workspace(B, Lmax) bytes.
 * wav_pack: packed [B * stride + n_fft] (stride % 4 == 0, stride >= ldw + n_fft; a multiple of hop makes the frames of
 * all items rows of ONE GEMM with ldx = hop): packed[b * stride + n_fft / 2 + j] = z[j] for j < wav_len[b], where z =
 * the trimmed item, (y / peak) * 0.95f in fp32 with an IEEE division if scaled[b] (an all-zero item with scaled[b] set
 * gives 0 / 0 = NaN samples, as numpy does; the padding stays zero); around it zeros, or with reflect the
 * signal mirrored about its first / last sample for n_fft / 2 samples on both sides (zeros where the item is too short
 * to supply them); zeros up to the next item and in the n_fft tail.  wav_out [B, ldw] (ldw % 4 == 0, ldw >= every
 * wav_len) = z, zero beyond wav_len[b].  n_fft % 8 == 0.
 * mel_project: spec [rows, ld_spec] split spectra (Re at 0.., Im at Fp.., Fp % 4 == 0, ld_spec >= 2 Fp), item b's frame
 * t at row b * rows_per_item + t -> mel [B, n_mels, Tmax]: mel[b, m, t] = sum over the bins of filter m, ascending, of
 * w * |X| (fp32 fma chain), then log(max(., 1e-5)) if log_clip; pad_value for t >= mel_len[b].  The basis is sparse:
 * meta [n_mels, 3] int32 = (first bin, number of bins, offset into w) per filter, w [nnz] fp32. */
size_t ft_wav_trim_peak_workspace(int B, long Lmax);
int ft_wav_trim_peak(const float* wav, long ld, const long* len, int B, long Lmax, int do_trim, float top_db,
                     int peak_norm, int hop, long* trim_start, long* trim_end, long* wav_len, long* mel_len, float* peak,
                     int* scaled, void* ws, void* stream);
int ft_wav_pack(const float* wav, long ld, const long* trim_start, const long* trim_end, const float* peak,
                const int* scaled, int B, float* packed, long stride, int n_fft, int reflect, float* wav_out, long ldw,
                void* stream);
int ft_mel_project(const float* spec, long ld_spec, int Fp, long rows_per_item, const long* mel_len, const float* w,
                   const int* meta, int nnz, int n_mels, int B, int Tmax, int log_clip, float pad_value, float* mel,
                   void* stream);

/* ---- sample-rate conversion in front of the audio front end (utils/dsp.py:40-42 DSP.load_wav = librosa.load(path,
 *      sr=sample_rate), which resamples every file on the way in) -------------------------------------------------- */
/* The polyphase design of scipy.signal.resample_poly (librosa res_type='polyphase'), for a ragged batch in the layout of
 * the front end above: x [B, ldx] fp32, len [B] int64 on the device, Lmax the host's bound.  For source_sr -> target_sr:
 * g = gcd, up = target_sr / g, down = source_sr / g, R = max(up, down) <= 1024, half = 10 R; in fp64
 * h[i] = (1/R) sinc((i - half) / R) kaiser(2 half + 1, 5.0)[i], h /= sum(h), h *= up, rounded to fp32 once.  For item b,
 * out_len[b] = ceil(len[b] * up / down) and, for n < out_len[b],
 *   y[b, n] = sum over k in [0, len[b]) with 0 <= half + n*down - k*up <= 2 half, ascending k, of
 *             h[half + n*down - k*up] * x[b, k]
 * as ONE fp32 fma chain (n*down in 64 bits); y[b, j] = 0 exactly for out_len[b] <= j < ldy.  Zero phase, zero padding on
 * both sides.  A term is left out by a select, never multiplied by zero, and nothing at k >= len[b] is loaded: NaN or
 * Inf in the padding of x or in another item changes no bit of an item, and an output's bits depend on its item and its
 * index alone -- not on B, Lmax, ldx, ldy or the item's position.
 * tab: the coefficients phase-major, [up][Tp] fp32 with T = ceil((2 half + 1) / up) taps per phase and the odd row
 * stride Tp = T | 1: tab[p * Tp + t] = h[p + t * up], 0 where p + t * up > 2 half, zero-filled up to
 * ft_resample_table_floats(up, down, half) floats (a multiple of 4; 0 = bad arguments), 16-byte aligned.
 * up == down is the identity (tab may be NULL): y[b, :len[b]] = x[b, :len[b]], out_len = len.
 * A len[b] outside [0, Lmax] is clamped into it (nothing indexes out of bounds) and sets *err_flag = 1 (int32 on the
 * device, zeroed by the caller; NULL = no report).  ldx % 4 == 0, ldy % 4 == 0, 1 <= Lmax <= ldx,
 * ldy >= ceil(Lmax * up / down), x and y 16-byte aligned.  One launch: a workgroup owns a tile of
 * ft_resample_tile(up, down, half) = 1024 consecutive outputs of one item (0 = bad arguments), grid (ceil(ldy / 1024), B).
 * ft_resample_route: which kernel the ratio takes -- 1: the table, the tile's input window and its outputs staged in LDS
 * (they fit 64 KiB: the pairs of standard rates down to about 4:1), 0: operands read through the cache (the same fma
 * chain, the same bits), 2: the identity copy, -1: bad arguments. */
int ft_resample_table_floats(int up, int down, int half);
int ft_resample_tile(int up, int down, int half);
int ft_resample_route(int up, int down, int half);
int ft_resample_poly_ragged(const float* x, long ldx, const long* len, int B, long Lmax, const float* tab, int up,
                            int down, int half, float* y, long ldy, long* out_len, int* err_flag, void* stream);

/* ---- durations from a Tacotron attention (duration_extraction/duration_extractor.py:23-84 DurationExtractor ;
 *      duration_extraction_pipe.py:56-62,173-183 ; utils/metrics.py:4-31 attention_score, r = 1) ---------------- */
/* One workgroup per item b; every length is read on the device.  Inputs: attn [B,Tm,Tx] fp32 (rows = mel frames),
 * mel [B,n_mels,Tmel] fp32, x [B,Tx_x] int64 tokens, x_len / mel_len [B] int64, sil_ids [n_sil] int64 (the token ids
 * that count as silent: pad + punctuation).  Item b uses attn[b, :mel_len, :x_len] and mel[b, :, :mel_len].
 * Frame i is silent if mean_c mel[c,i] < silence_threshold; if at least two frames are silent, the attention of every
 * silent frame gets +shift on silent tokens and -shift on the others; then clamp [0,1] and cost = 1 - att.  The
 * cheapest right / down / diagonal path from (0,0) to (mel_len-1, x_len-1) (an edge weighs the cost of the cell it
 * enters, distances summed in fp64; exact ties: diagonal, then down, then right) gives each frame to the last token
 * its row visits.  Outputs: durations [B,Tx_out] int64 (0 at j >= x_len); fstats [B,3] fp64 = (mean clamped attention
 * along the path over non-silent frames -- NaN if every frame is silent --, align score = fraction of consecutive
 * frames whose argmax token moves by <= 1 (fp32; NaN for one frame), path cost); istats [B,3] int64 = (max duration,
 * longest run of ones, status: 0 ok, 1 bad x_len, 2 bad mel_len, 3 no workspace; a bad item writes zero durations).
 * x_len <= min(Tx, Tx_x, Tx_out) and Tx <= 1024.  ws: ft_dur_workspace(B, Tm, Tx) bytes. */
size_t ft_dur_workspace(int B, int Tm, int Tx);
int ft_dur_extract(const float* attn, int Tm, int Tx, const float* mel, int n_mels, int Tmel, const long* x, int Tx_x,
                   const long* x_len, const long* mel_len, const long* sil_ids, int n_sil, float silence_threshold,
                   float silence_prob_shift, int B, long* durations, int Tx_out, double* fstats, long* istats,
                   void* ws, void* stream);

/* ---- per-token pitch and energy (train_tacotron.py:39-93 extract_pitch_energy ; :24-35 normalize_values) ---------- */
/* One workgroup per item b; every length is read on the device.  Inputs: log mel [B,n_mels,Tmel] fp32, mel_len [B]
 * int64; raw pitch [B,Tp] fp32 and pitch_len [B] int64 (item b's track is pitch[b, :pitch_len]); dur [B,Tx] int64,
 * x_len [B] int64.  energy[t] = ||exp(mel[:, t])||_2 (:62; fp32, channels added in ascending order, each square
 * rounded before its add).  Token j < min(mel_len, x_len) covers frames [cum_j, cum_j + dur_j) (:65-73): pitch_tok =
 * mean of the raw pitch there without zeros and values outside [pitch_min_freq, pitch_max_freq] (inclusive; frames
 * past pitch_len count as dropped), energy_tok = mean of the frame energies; both summed in fp64 and rounded once, 0
 * for an empty segment and for every j >= min(mel_len, x_len).  status [B] int32: 0 ok, 1 durations do not sum to
 * mel_len (:63: the item is skipped), 2 bad x_len (1..Tx), 3 bad mel_len (1..Tmel), 4 bad pitch_len (0..Tp),
 * 5 negative duration, 6 no workspace; an item with status != 0 gets zeros.  Tx <= 2048; ws:
 * ft_token_values_workspace(B, Tmel) bytes (0 for Tmel <= 8192: the frame values then sit in LDS; NULL allowed). */
size_t ft_token_values_workspace(int B, int Tmel);
int ft_token_values(const float* mel, int n_mels, int Tmel, const long* mel_len, const float* pitch, int Tp,
                    const long* pitch_len, const long* dur, int Tx, const long* x_len, float pitch_min_freq,
                    float pitch_max_freq, int B, float* pitch_tok, float* energy_tok, int* status, void* ws,
                    void* stream);
/* normalize_values over one speaker's token pitches values[n] (the caller keeps them in a fixed item order), in place:
 * count, mean and population std of the nonzero values in fp64 (two passes, fixed-order slabs, no atomics), then
 * mean32 = (float)mean, std32 = (float)std, std32 = 1e10 unless std32 > 0 (:28-29; no nonzero value: mean NaN), and
 * v = (v - mean32) / std32 in fp32 where v != 0 (zeros stay 0).  stats [5] fp64 = (count, mean, std, mean32, std32),
 * not written for n == 0.  Three launches; ws: ft_pitch_norm_workspace(n) bytes. */
size_t ft_pitch_norm_workspace(long n);
int ft_pitch_norm(float* values, long n, double* stats, void* ws, void* stream);

/* ---- Tacotron teacher-forced attention recurrence (models/tacotron.py:124-146 Decoder.forward, :65-99 LSA) -------- */
/* All S decoder steps of attn_rnn (GRUCell 384 -> 256, gates r, z, n) + LSA (location conv 2 -> 32, k = 31, pad 15, no
 * bias; L 32 -> 256; W 256 -> 256; v 256 -> 1; softmax over all Tx columns, no mask) + context = scores @ enc_pq, three
 * launches per step on `stream` (csrc/ft_taco.hip).  Inputs: enc_proj / enc_pq [B,Tx,256]; P [S,B,768] = the prenet
 * half of the GRU input projection, b_ih included; w_ih = attn_rnn.weight_ih [768, ld_w_ih] (its columns 0..255, the
 * context's, are read); w_hh [768,256], b_hh [768]; W [256,256], b_W, conv_w [32,2,31], L [256,32], b_L, v [256].
 * Output attn [B,S,Tx].  hist (optional, NULL to skip) [S,B,512]: row (s,b) = [context_s | h_attn_s], the rnn_input
 * operand of the mel path.  Zero initial states; the LSA state lives in the workspace for the call only.  Weights,
 * hist and ws 16-byte aligned.  1 <= Tx <= 1024, S >= 1; ws: ft_taco_attend_workspace(B, Tx) bytes (0: bad dims). */
size_t ft_taco_attend_workspace(int B, int Tx);
int ft_taco_attend(const float* enc_proj, const float* enc_pq, const float* P, const float* w_ih, long ld_w_ih,
                   const float* w_hh, const float* b_hh, const float* W, const float* b_W, const float* conv_w,
                   const float* L, const float* b_L, const float* v, float* attn, float* hist, int B, int Tx, int S,
                   void* ws, size_t ws_bytes, void* stream);
/* teacher-forced prenet inputs: out [S,B,n_mels] (time-major), out[0] = 0, out[i] = mel[:, :, i*r - 1] of mel
 * [B,n_mels,Tm]; requires (S-1)*r <= Tm */
int ft_taco_frames(const float* mel, int B, int n_mels, int Tm, int r, int S, float* out, void* stream);
/* out = x + y over n floats (the decoder's residual adds) */
int ft_taco_add(const float* x, const float* y, float* out, long n, void* stream);

/* ---- Tacotron teacher training: attention BPTT and the zoneout LSTMCells (csrc/ft_taco_train.hip) ---------------- */
/* Backward of ft_taco_attend (models/tacotron.py:124-146, :65-99), s = S-1 .. 0, five plain launches per step, then the
 * factorised weight gradients on ft_linear_bwd_weight / ft_colsum.  Inputs: ft_taco_attend's operands; hist [S,B,512]
 * and attn [B,S,Tx] as it wrote them; dhist [S,B,512] = the gradient of the [context | h_attn] rows.  attn itself gets
 * no gradient (the trainer only scores it).  The cumulative attention is rebuilt as a prefix sum of attn, tanh and the
 * GRU gates are recomputed.  Outputs (every element written): dep, depq [B,Tx,256] (gradients of enc_proj / enc_pq);
 * dP [S,B,768]; dw_ih_ctx [768,256] = the gradient of w_ih[:, :256]; dw_hh [768,256]; db_hh [768]; dW [256,256];
 * dbW, dbL [256] (equal); dconv_w [32,2,31]; dL [256,32]; dv [256].  No atomics, fixed summation order: one input
 * gives one output bit pattern.  enc_pq, the weights, hist, depq, dP and ws 16-byte aligned.  1 <= Tx <= 1024, B >= 1,
 * S >= 1; ws: ft_taco_attend_bwd_workspace(B, Tx, S) bytes (0: bad dims). */
size_t ft_taco_attend_bwd_workspace(int B, int Tx, int S);
int ft_taco_attend_bwd(const float* enc_proj, const float* enc_pq, const float* P, const float* w_ih, long ld_w_ih,
                       const float* w_hh, const float* b_hh, const float* W, const float* b_W, const float* conv_w,
                       const float* L, const float* b_L, const float* v, const float* hist, const float* attn,
                       const float* dhist, float* dep, float* depq, float* dP, float* dw_ih_ctx, float* dw_hh,
                       float* db_hh, float* dW, float* dbW, float* dconv_w, float* dL, float* dbL, float* dv, int B,
                       int Tx, int S, void* ws, size_t ws_bytes, void* stream);
/* nn.LSTMCell over S steps from zero states with the reference's zoneout (models/tacotron.py:119-122, :152-166):
 * h_s = m_s h_{s-1} + (1 - m_s) cell(x_s, (h_{s-1}, c_{s-1})).h, c_s = the cell's c (not zoned); the zoned h_s is the
 * output and the next step's recurrent input.  m_s[b,u] = 1 exactly where ft_dropout's mask of (p, seed) is 0 at flat
 * index (s B + b) L + u of [S,B,L], no rescaling; p = 0 zones nothing, p = 1 everything (ft_dropout's seed contract).
 * One launch per step.  fwd: xp [S,B,4L] = x W_ih^T + b_ih (gates i, f, g, o), w_hh [4L,L], b_hh [4L] -> gates [S,B,4L]
 * (activated), c, h [S,B,L].  bwd: dout [S,B,L] = the gradient of h, w_hhT [L,4L] = w_hh^T -> dxp [S,B,4L], the
 * gradient of the pre-activations (dw_hh = dxp^T h_{s-1}, db = column sums, dx = dxp W_ih follow on the GEMM kernels).
 * L % 4 == 0, B >= 1, S >= 1; w_hh, w_hhT, h and dxp 16-byte aligned; ws: ft_taco_lstm_zone_workspace(B, L) bytes. */
size_t ft_taco_lstm_zone_workspace(int B, int L);
int ft_taco_lstm_zone_fwd(const float* xp, const float* w_hh, const float* b_hh, float p, uint64_t seed, float* gates,
                          float* c, float* h, int B, int S, int L, void* stream);
int ft_taco_lstm_zone_bwd(const float* dout, const float* gates, const float* c, const float* w_hhT, float p,
                          uint64_t seed, float* dxp, int B, int S, int L, void* ws, size_t ws_bytes, void* stream);
/* PreNet layer backward (models/tacotron.py:29-45: fc -> ReLU -> dropout): y = the layer's stored output, 0 where the
 * ReLU clipped or the dropout dropped -> dz = y > 0 ? dy / (1 - p) : 0, the gradient of the Linear's output; 0 <= p < 1 */
int ft_relu_dropout_bwd(const float* dy, const float* y, float* dz, long n, float p, void* stream);
/* mel_proj weight gradient (models/tacotron.py:169-170): dwp [r * n_mels, L], packed rows k * n_mels + n (the rows the
 * [:, :, :r] slice keeps) -> dw [n_mels * max_r, L] at rows n * max_r + k, exact zeros in the rows with k >= r */
int ft_taco_mel_scatter(const float* dwp, float* dw, int n_mels, int max_r, int r, int L, void* stream);

/* ---- Tacotron autoregressive generate (models/tacotron.py:283-349 Tacotron.generate, :124-174 Decoder.forward) --- */
/* Decoder steps [s0, s0 + n) of generate at B = 1 in eval mode (no dropout, no zoneout), eight launches per step on
 * `stream` (csrc/ft_taco.hip), all enqueued here: decoder prenet (fc1 80 -> 256, fc2 256 -> 128, ReLU) of the last
 * frame of step s-1 (zeros at s = 0) and the prenet half of the GRU input projection -> P[s]; the attention GRU, LSA
 * and context (ft_taco_attend's kernels); rnn_input; res_rnn1 and res_rnn2 (nn.LSTMCell, gates i, f, g, o, each plus
 * its input); mel_proj rows n*20 + k, k < r (the [:, :, :r] slice).  s0 == 0 starts from zero states and sets
 * *s_out = S; a later call continues from the workspace, which must not be touched in between.  Stop rule (:336): the
 * first step s whose 80 r frames are all < stop_threshold (fp32, NaN never is) with s*r > 10 sets *s_out = s + 1;
 * steps after it still run but only write slots >= *s_out.
 * Inputs: enc_proj / enc_pq [1,Tx,256]; fc1_w [256,80], fc1_b, fc2_w [128,256], fc2_b; w_ih = attn_rnn.weight_ih
 * [768, ld_w_ih] (context columns 0..255, prenet columns 256..383), b_ih, w_hh [768,256], b_hh; the LSA weights as
 * ft_taco_attend; rnn_in_w [L,512], rnn_in_b [L]; r*_w_ih / r*_w_hh [4L,L], r*_b_ih / r*_b_hh [4L]; mel_w [1600,L]
 * (L = lstm_dims).  Outputs, slots for all S = ceil(steps / r) steps: P [S,768]; hist [S,512] = [context | h_attn];
 * attn [1,S,Tx]; frames [S*r,80] (channels last, frame s*r + k); s_out one device int.  Weights, hist and ws 16-byte
 * aligned.  1 <= Tx <= 1024, 1 <= r <= 20, 0 <= s0, s0 + n <= S; ws: ft_taco_gen_workspace(Tx, lstm_dims, r) bytes
 * (0: bad dims).  Fixed summation order, no atomics on values: one input gives one output bit pattern, whatever the
 * split into calls. */
size_t ft_taco_gen_workspace(int Tx, int lstm_dims, int r);
int ft_taco_gen_steps(const float* enc_proj, const float* enc_pq, const float* fc1_w, const float* fc1_b,
                      const float* fc2_w, const float* fc2_b, const float* w_ih, long ld_w_ih, const float* b_ih,
                      const float* w_hh, const float* b_hh, const float* W, const float* b_W, const float* conv_w,
                      const float* L, const float* b_L, const float* v, const float* rnn_in_w, const float* rnn_in_b,
                      const float* r1_w_ih, const float* r1_w_hh, const float* r1_b_ih, const float* r1_b_hh,
                      const float* r2_w_ih, const float* r2_w_hh, const float* r2_b_ih, const float* r2_b_hh,
                      const float* mel_w, float stop_threshold, float* P, float* hist, float* attn, float* frames,
                      int* s_out, int Tx, int lstm_dims, int r, int S, int s0, int n, void* ws, size_t ws_bytes,
                      void* stream);

/* ---- Tacotron generate of a ragged batch (Tacotron.generate_batch) --------------------------------------------- */
/* ft_taco_gen_steps for B sentences at once, item b with lens[b] tokens (int64 [B], device, 1 <= lens[b] <= Tx; a
 * value outside is clamped into that range, the caller reports it).  Item b gets what ft_taco_gen_steps gives the
 * sentence alone at Tx = lens[b]: energies, softmax, LSA state and context stop at lens[b], no row of enc_proj / enc_pq
 * at t >= lens[b] is read, and attn is exactly 0 there.  Eight launches per step (csrc/ft_taco.hip); the decoder cells
 * run as [16 items x K] x [K x 16 columns] products on the f32 MFMA, so a tile of 16 items reads each weight once per
 * step.  The weights are those of ft_taco_gen_steps.  Layouts: enc_proj / enc_pq [B,Tx,256]; P [S,B,768]; hist
 * [S,B,512] = [context | h_attn]; attn [B,S,Tx]; frames [B,S*r,80] (channels last, frame s*r + k); s_out int32 [B].
 * s0 == 0 starts from zero states and sets s_out[b] = S; a later call continues from the workspace.  Stop rule, per
 * item: the first step s whose 80 r values of item b are all < stop_threshold (NaN never is) with s*r > 10 sets
 * s_out[b] = s + 1.  Every item is stepped for all n steps, stopped or not; slots at s >= s_out[b] are written and mean
 * nothing.  No sum crosses items.  Alignment, bounds on Tx, r, s0, n as ft_taco_gen_steps; 1 <= B <= 65535; ws:
 * ft_taco_gen_batch_workspace(B, Tx, lstm_dims, r) bytes (0: bad dims).  Fixed summation order, no atomics on values. */
size_t ft_taco_gen_batch_workspace(int B, int Tx, int lstm_dims, int r);
int ft_taco_gen_batch_steps(const float* enc_proj, const float* enc_pq, const float* fc1_w, const float* fc1_b,
                            const float* fc2_w, const float* fc2_b, const float* w_ih, long ld_w_ih, const float* b_ih,
                            const float* w_hh, const float* b_hh, const float* W, const float* b_W,
                            const float* conv_w, const float* L, const float* b_L, const float* v,
                            const float* rnn_in_w, const float* rnn_in_b, const float* r1_w_ih, const float* r1_w_hh,
                            const float* r1_b_ih, const float* r1_b_hh, const float* r2_w_ih, const float* r2_w_hh,
                            const float* r2_b_ih, const float* r2_b_hh, const float* mel_w, float stop_threshold,
                            float* P, float* hist, float* attn, float* frames, int* s_out, const long* lens, int B,
                            int Tx, int lstm_dims, int r, int S, int s0, int n, void* ws, size_t ws_bytes,
                            void* stream);

/* ---- raw pitch of a ragged batch: pYIN (pitch_extraction/pitch_extractor.py:24-47 LibrosaPitchExtractor) --------- */
/* Probabilistic YIN (Mauch & Dixon 2014) with librosa.pyin's documented defaults, in three launches (csrc/ft_pitch.hip);
 * the full definition is DESIGN.md section 7, the numpy restatement tests/pyin_cpu.py, the host tables
 * forwardtacotron_amd/pitch.py pyin_tables.  With W = frame_length / 2: pmin = max(floor(sr / fmax), 1), pmax =
 * min(ceil(sr / fmin), frame_length - W - 1), P = pmax - pmin + 1 periods; N = floor(120 log2(fmax / fmin)) + 1 pitch
 * bins; half = 5 round(35.92 * 12 * hop / sr), a transition band of 2 half + 1 bins.  Item b has T_b = 1 + len_b / hop
 * frames (wav_to_mel's mel_len); frame t is frame_length samples from t * hop of the wav zero-padded by
 * frame_length / 2 on both sides.  Every entry reads its lengths on the device and clamps them (wav_len into [0, Lmax],
 * frames into [0, Tmax]; the Viterbi into [1, Tmax]); nothing past a length is loaded; nothing is sized from device
 * values and nothing synchronises.  Limits: frame_length even and >= 4; the samples of four frames and their difference
 * functions sit in LDS, ft_pyin_cmnd_lds(...) bytes <= 65536 (0: bad arguments); P <= 1024; N <= 1024, i.e. at most
 * 2N = 2048 HMM states (two per thread of the Viterbi's 1024), half <= 2048, and the Viterbi's LDS plan -- (4N + 6 half +
 * 33) floats, 2N flag bytes and at least one row of 2N 16-bit back-pointers -- within 65536 bytes: ft_pyin_viterbi_rows(N,
 * half) is the number of back-pointer rows it holds (at most 32), 0 where N or half is out of range or no row fits (N =
 * 1024 fits up to half = 1786).
 *
 * ft_pyin_cmnd: wav [B, ld] fp32, wav_len [B] int64 -> dn [B, Tmax, P] fp32, Tmax = 1 + Lmax / hop, and frames [B]
 * int64 = T_b.  d(tau) = sum_{j < W} (x_j - x_{j+tau})^2 for tau = 0 .. pmax, formed directly in fp32 (one ascending fma
 * chain per tau, the same whatever the batch); c(tau) = (sum_{u = 1 .. tau} d(u)) / tau; dn[tau - pmin] = d(tau) /
 * max(c(tau), FLT_MIN).  A frame of zeros and every frame t >= T_b give exactly 0.
 *
 * ft_pyin_observe: dn, frames -> lo_v [B, Tmax, N], lo_u [B, Tmax], vp [B, Tmax].  Host tables, float64 rounded once:
 * thr[k] = (k + 1) / 100, bp[k] = F((k + 1) / 100) - F(k / 100) of the Beta(2, 18) cdf F, k = 0 .. 99; bpc[m] = sum of
 * bp[0 .. m - 1], m = 0 .. 100; E[pos] = exp(-2 pos), C[n] = (1 - exp(-2)) / (1 - exp(-2 n)) (C[0] = 0), nE >= (P + 1) /
 * 2 + 1 entries each; LZ = log(FLT_MIN).  Trough i: dn[i] < dn[i-1] and dn[i] <= dn[i+1] (ends: strictly below the one
 * neighbour).  p_i = sum over k ascending of [h_i < thr[k]] (E[pos(i,k)] * C[n(k)]) * bp[k] in fp32, pos / n = troughs
 * below thr[k] before i / in all; the lowest trough g of minimal height gets p_g += 0.01f * bpc[m], m = the number of k
 * with h_g >= thr[k].  A trough with p_i > 0 is a candidate at period pmin + i + shift (parabolic shift -b / a if |b| <
 * |a| else 0, 0 at both ends) and bin floor(120 log2(f0 / fmin) + 0.5), both formed in fp64 from the fp32 dn; bin < 0
 * becomes 0, bin > N - 1 drops the candidate, the larger i wins a shared bin.  vp = clamp(sum of the bins' p, 0, 1);
 * lo_v = log(max(p, FLT_MIN)) (LZ itself where p is 0), lo_u = log(max((1 - vp) / N, FLT_MIN)).  A frame t >= frames[b]
 * is treated as dn = 0: lo_v = LZ, vp = 0.  Optional outputs for tests (NULL to skip): prob [B, Tmax, P] = p_i, -1 where
 * i is no trough; info [B, Tmax, 102] int32 = (g or -1, m, n(0) .. n(99)); pos [B, Tmax, P, 100] int16 = pos(i, k) where
 * trough i is below thr[k], -1 where it is not or i is no trough (so pos >= 0 is `below`).
 *
 * ft_pyin_viterbi: lo_v, lo_u, frames -> state [B, Tmax] int32, score [B], pitch [B, Tmax].  States: voiced bins
 * 0 .. N-1, then unvoiced N .. 2N-1.  Host tables: logtri [2 half + 1] = log of the triangle window, lognorm [N] = log of
 * its sum over the targets inside [0, N), freqs [N] = fmin 2^(s / 120); ls = log .99, lw = log .01, LZ, lN = -log N.  Every
 * operation is one fp32 add, subtract or maximum: t = 0: delta_v[s] = LZ + lo_v[0, s], delta_u[s] = lN + lo_u[0]; t >= 1:
 * a[k] = max(delta_v[k] + ls, delta_u[k] + lw) - lognorm[k], delta'_v[s] = max over |s - k| <= half of (a[k] + logtri[s -
 * k + half]) + lo_v[t, s]; the unvoiced targets take max(delta_v[k] + lw, delta_u[k] + ls) and add lo_u[t]; after every
 * step, t = 0 included, the maximum over all 2N states is subtracted.  score = the fp32 running sum of the subtracted
 * maxima in step order (the final maximum is 0 after the normalisation, so this is the path's log score).  Ties inside a
 * step go to the lowest source state; the path is traced back from the lowest maximal final state.  pitch[t] =
 * freqs[state] for a voiced state, 0 for an unvoiced one; at t >= T_b state is -1 and pitch 0.  An item with NaN in its
 * observations finishes like any other (every loop is bounded by Tmax and N); its path is a valid state sequence of no
 * meaning and its score NaN.  ws: ft_pyin_viterbi_workspace(B, Tmax, N) bytes (16-bit back-pointers [B, Tmax, 2N]; 0:
 * bad dims). */
size_t ft_pyin_cmnd_lds(int frame_length, int hop, int pmin, int pmax);
int ft_pyin_cmnd(const float* wav, long ld, const long* wav_len, int B, long Lmax, int frame_length, int hop, int pmin,
                 int pmax, int Tmax, float* dn, long* frames, void* stream);
int ft_pyin_observe(const float* dn, const long* frames, int B, int Tmax, int P, int pmin, int N, double sr, double fmin,
                    const float* thr, const float* bp, const float* bpc, const float* E, const float* C, int nE, float LZ,
                    float* lo_v, float* lo_u, float* vp, float* prob, int* info, short* pos, void* stream);
int ft_pyin_viterbi_rows(int N, int half);
size_t ft_pyin_viterbi_workspace(int B, int Tmax, int N);
int ft_pyin_viterbi(const float* lo_v, const float* lo_u, const long* frames, int B, int Tmax, int N, int half,
                    const float* logtri, const float* lognorm, const float* freqs, float ls, float lw, float LZ, float lN,
                    int* state, float* score, float* pitch, void* ws, size_t ws_bytes, void* stream);

/* ---- speaker embeddings (preprocess.py:80,173-182,218-227: resemblyzer's VoiceEncoder.embed_utterance per file and the
 *      mean per speaker; speaker.VoiceEncoder; the definition is DESIGN.md section 7, "Speaker embedding") ------------ */
/* A ragged batch as for the audio front end: wav [B, ld] fp32 (16-byte aligned rows, ld % 4 == 0), len [B] int64 on the
 * device, 1 <= len[b] <= Lmax <= ld.  A len[b] outside [1, Lmax] is clamped into it and ft_spk_gain sets *err_flag = 1
 * (int32 on the device, zeroed by the caller; NULL = no report).
 * The slice rule (ft_spk_slices on the host; the kernels apply the same function to len[b] on the device): with hop,
 * partial_frames pf, frame_step and min_coverage = cov_num / cov_den (0 <= cov_num <= cov_den <= 2^20), n_frames =
 * ceil((n + 1) / hop), steps = max(1, n_frames - pf + frame_step + 1), one partial [i, i + pf) in frames per i in
 * range(0, steps, frame_step); the last one is dropped if it is not the only one and (n - i hop) cov_den < cov_num pf hop.
 * count = the partials kept, frames = i_last + pf = the mel frames they cover.
 * ft_spk_gain (one workgroup per item): ms = (sum of w^2 over the item's samples, in fp64 and in an order that depends on
 * len[b] alone) / len[b]; with normalize, gain[b] = g = target / sqrt(ms) rounded to fp32 once if g > 1, else 1 (also
 * for ms == 0 or NaN); without, 1.  n_partials[b], frames[b] = the slice rule at len[b].
 * ft_spk_pack: packed [B * stride + n_fft] (stride % 4 == 0, n_fft % 8 == 0): packed[b * stride + n_fft / 2 + j] =
 * gain[b] * wav[b, j] (one fp32 multiplication) for j < len[b] where that lies inside the item's stride, zeros elsewhere
 * and in the n_fft tail.  With stride a multiple of hop the frames of all items are rows of ONE GEMM with ldx = hop.
 * ft_spk_mel_power: spec [B * rows_per_item, ld_spec] split spectra (Re at 0.., Im at Fp.., Fp % 4 == 0) -> mel [B *
 * rows_per_item, n_mels] FRAME-major: mel[row, m] = sum over the bins of filter m, ascending, of w * (Re^2 + Im^2) (fp32
 * fma chain; no square root, no log); rows t >= frames[b] of item b are zero.  The basis is ft_mel_project's sparse form
 * (meta [n_mels, 3] int32 = first bin, number of bins, offset into w [nnz]).
 * ft_spk_gather_partials: table [P, 2] int32 = (item, first frame) per slot -> out [pf, P, n_mels] TIME-major:
 * out[t, p, :] = mel[item * rows_per_item + first + t, :] if first + pf <= frames[item], else zero (an unused slot).
 * ft_spk_segment_mean_norm: rows [N, E] (E <= 1024); segment s is the entries offsets[s] .. offsets[s + 1] - 1 (int64
 * [S + 1]) of index (int64; NULL: the rows themselves, contiguous), cut to its first count[s] entries where count (int64
 * [S]) is not NULL.  With normalize_rows every row of a segment is first divided by its own 2-norm (and written to
 * rows_out [N, E] where that is not NULL; rows of no segment are not written).  out[s] = m / |m|_2, m = (sum of the
 * segment's rows in ascending order) / their number.  No epsilon: a zero norm, or an empty segment, gives NaN. */
int ft_spk_slices(long n, int hop, int partial_frames, int frame_step, long cov_num, long cov_den, long* count,
                  long* frames);
int ft_spk_gain(const float* wav, long ld, const long* len, int B, long Lmax, double target, int hop, int partial_frames,
                int frame_step, long cov_num, long cov_den, int normalize, float* gain, long* n_partials, long* frames,
                int* err_flag, void* stream);
int ft_spk_pack(const float* wav, long ld, const long* len, int B, long Lmax, const float* gain, float* packed,
                long stride, int n_fft, void* stream);
int ft_spk_mel_power(const float* spec, long ld_spec, int Fp, int rows_per_item, const long* frames, const float* w,
                     const int* meta, int nnz, int n_mels, int B, float* mel, void* stream);
int ft_spk_gather_partials(const float* mel, int rows_per_item, int n_mels, const long* frames, const int* table, int P,
                           int partial_frames, int B, float* out, void* stream);
int ft_spk_segment_mean_norm(const float* rows, int N, int E, const long* index, const long* offsets, const long* count,
                             int S, int normalize_rows, float* out, float* rows_out, void* stream);

/* ---- MelGAN vocoder (notebook_utils/synthesize.py:46-48: the hub generator's inference(mel_post); melgan.MelGAN; the
 *      definition is DESIGN.md section 7, "MelGAN vocoder") ----------------------------------------------------------- */
/* A ragged batch of mels: len [B] int64 on the device, 1 <= len[b] <= Tmax (clamped into that range; ft_melgan_conv_in
 * sets *err_flag = 1 for a length outside it, NULL = no report); len == NULL: every item has Tmax frames.  `tail` frames
 * of pad_value are appended to every item (10 in inference, 0 in forward).  Activations are channels-last [row, C] fp32;
 * at upsampling `scale` item b owns rows [b (Tmax + tail) scale, (b + 1) (Tmax + tail) scale) and rows at >= L = (len[b] +
 * tail) scale are neither written nor read.  Reflection is per item: row -j is row j, row L - 1 + j is row L - 1 - j.
 * Widths are multiples of 8.  Weights are packed [k][CP] fp32 with CP = the output width rounded up to 32 and zeros in
 * the added columns; biases are [CP], zero-padded likewise.  All products are exact-fp32 MFMA fma chains.
 * ft_melgan_tile_rows(kind, c): the rows per workgroup tile the plan gives width c (kind 0: conv_in, c = n_mels; 1:
 * upsample, c = cin, in INPUT rows; 2: resblock; 3: conv_out, in samples); 0 where the width is not supported.
 * ft_melgan_conv_in: mel [B, n_mels, Tmax] as it is -> out [B (Tmax + tail), cout]: Conv1d(k = 7) over the reflection by 3
 *   of x[t] = (mel[t] + 5) / 5 (t < len[b]) and (pad_value + 5) / 5 (the tail); w [7][n_mels][CP].  n_mels <= 128.
 * ft_melgan_upsample: LeakyReLU(0.2), ConvTranspose1d(cin, cout, k = 2 stride, stride, padding = stride / 2), stride
 *   even: x at `scale` -> out at scale * stride; w [2 stride][cin][CP] with w[j][ci][co] = weight[ci][co][j].  cin <= 512.
 * ft_melgan_resblock: out = shortcut(x) + conv1x1(lrelu(conv3 at `dilation` (reflect(lrelu(x))))), all three biases; w1
 *   [3][ch][CP], w2 and ws [ch][CP] (w[ci][co] = weight[co][ci]); x != out.  ch <= 256, dilation <= 9.
 * ft_melgan_conv_out: LeakyReLU, reflect 3, Conv1d(ch, 1, k = 7), tanh: x at `scale` -> wav [B, Tmax scale], exactly 0 at
 *   j >= len[b] scale (the tail's samples are dropped), and wav_i16 = truncate(clamp(32768 wav, -32768, 32767)) in the
 *   same pass; w [ch][32] with column = tap.  ch <= 32. */
int ft_melgan_tile_rows(int kind, int c);
int ft_melgan_conv_in(const float* mel, const long* lens, int B, int n_mels, int Tmax, int tail, float pad_value,
                      const float* w, const float* bias, int cout, float* out, int* err_flag, void* stream);
int ft_melgan_upsample(const float* x, const long* lens, int B, int Tmax, int tail, int scale, int cin, int cout,
                       int stride, const float* w, const float* bias, float* out, void* stream);
int ft_melgan_resblock(const float* x, const long* lens, int B, int Tmax, int tail, int scale, int ch, int dilation,
                       const float* w1, const float* b1, const float* w2, const float* b2, const float* ws,
                       const float* bs, float* out, void* stream);
int ft_melgan_conv_out(const float* x, const long* lens, int B, int Tmax, int tail, int scale, int ch, const float* w,
                       float bias, float* wav, short* wav_i16, void* stream);

/* ---- HiFi-GAN vocoder (gen_forward.py:31-37,109-116: the third vocoder target; hifigan.HiFiGAN; the definition is
 *      DESIGN.md section 7, "HiFi-GAN vocoder") ---------------------------------------------------------------------- */
/* The layout, the lengths and the packing are MelGAN's above with tail = 0 and ZERO edges instead of reflection: rows
 * outside an item's [0, L), L = len[b] scale, are zeros, and rows at >= L are neither written nor read.
 * ft_hifigan_tile_rows(kind, c): rows per workgroup tile for width c (kind 0: conv_in, c = n_mels; 1: upsample, c = cin,
 *   in INPUT rows; 2: resconv; 3: conv_out, in samples; 4: respair, in rows of the intermediate -- a tile's output is
 *   that minus k - 1); 0 where the width is not supported.
 * ft_hifigan_conv_in: mel [B, n_mels, Tmax] as it is, no normalisation -> out [B Tmax, cout]: Conv1d(k = 7, padding 3);
 *   w [7][n_mels][CP].  n_mels <= 128.
 * ft_hifigan_upsample: LeakyReLU(0.1), ConvTranspose1d(cin, cout, k = 2 stride, stride, padding = stride / 2), stride
 *   even: x at `scale` -> out at scale * stride; w [2 stride][cin][CP].  cin <= 512.
 * ft_hifigan_resconv: out = res + bias + Conv1d(ch, ch, k, dilation, padding = dilation (k - 1) / 2)(lrelu_0.1(x)); w
 *   [k][ch][CP]; k odd <= 11, dilation (k - 1) / 2 <= 40, ch <= 256, x != out.  res_mode 0: no res; 1: res = x; 2: res
 *   [rows, ch] from memory.  acc_mode 0: out = value; 1: out += value; 2: out = (out + value) / nk (the average over a
 *   stage's nk parallel blocks: launches on one stream, block 0 stores, later ones add, the last divides).
 * ft_hifigan_respair: ResBlock1's pair in one launch, out = x + b2 + Conv1d(k, padding (k - 1) / 2)(lrelu(b1 + Conv1d(k,
 *   dilation)(lrelu(x)))), the intermediate zero outside [0, L) and kept in LDS; acc_mode as above.  ch <= 64, dilation
 *   (k - 1) / 2 <= 25.
 * ft_hifigan_conv_out: LeakyReLU(0.01), Conv1d(ch, 1, k = 7, padding 3), tanh: x at `scale` -> wav [B, Tmax scale],
 *   exactly 0 at j >= len[b] scale, and wav_i16 = truncate(clamp(32768 wav, -32768, 32767)); w [ch][32], column = tap.
 *   ch <= 32. */
int ft_hifigan_tile_rows(int kind, int c);
int ft_hifigan_conv_in(const float* mel, const long* lens, int B, int n_mels, int Tmax, const float* w, const float* bias,
                       int cout, float* out, int* err_flag, void* stream);
int ft_hifigan_upsample(const float* x, const long* lens, int B, int Tmax, int scale, int cin, int cout, int stride,
                        const float* w, const float* bias, float* out, void* stream);
int ft_hifigan_resconv(const float* x, const long* lens, int B, int Tmax, int scale, int ch, int k, int dilation,
                       const float* w, const float* bias, const float* res, int res_mode, int acc_mode, int nk, float* out,
                       void* stream);
int ft_hifigan_respair(const float* x, const long* lens, int B, int Tmax, int scale, int ch, int k, int dilation,
                       const float* w1, const float* b1, const float* w2, const float* b2, int acc_mode, int nk, float* out,
                       void* stream);
int ft_hifigan_conv_out(const float* x, const long* lens, int B, int Tmax, int scale, int ch, const float* w, float bias,
                        float* wav, short* wav_i16, void* stream);

/* ---- HiFi-GAN's residual convolution with fp16 matrix operands (hifigan.HiFiGAN.matmul_dtype = 'fp16'; csrc/
 *      ft_hifigan_h16.hip; the arithmetic is DESIGN.md section 7, "fp16 mode") --------------------------------------- */
/* ft_hifigan_resconv_h16: ft_hifigan_resconv's contract, arguments and limits with a = fp16(clamp(lrelu_0.1(x), +-65504))
 *   and fp16 weights on v_mfma_f32_32x32x16_f16, fp32 accumulation from the fp32 bias, the residual (res_mode 1: x itself)
 *   added in fp32 from memory.  x, bias, res, out fp32 as there; w: fp16 [k][cpad / 8][CP][8], cpad = ch rounded up to 16,
 *   element [tap][c / 8][co][c % 8] = W[co][c][tap], zeros at c >= ch and co >= ch; 16-byte aligned.
 * ft_hifigan_h16_plan(field, c): its launch plan for width c (csrc/ft_voc_plan_h16.h, host-only).  field 0: rows per
 *   workgroup tile; 1: static LDS bytes; 2: threads; 3: the staged width of the arrangement; 4: cpad.  0 where the width
 *   is not supported (multiples of 8 in 8..256); an unknown field answers -1. */
int ft_hifigan_h16_plan(int field, int c);
int ft_hifigan_resconv_h16(const float* x, const long* lens, int B, int Tmax, int scale, int ch, int k, int dilation,
                           const void* w, const float* bias, const float* res, int res_mode, int acc_mode, int nk, float* out,
                           void* stream);

/* ---- the GAN vocoders' launch plan (csrc/ft_voc_plan.h, host-only) ------------------------------------------------------ */
/* ft_voc_plan(field, a, b, c): one value of the plan both vocoders launch by; host-only, no device is touched.  field 0:
 * residual taps at most (11); 1: resconv halo at most (40); 2: respair first-convolution halo at most (25); 3: 1 where
 * ResBlock1's pair at width a, k = b taps, dilation c runs as ONE ft_hifigan_respair launch, 0 where it runs as two
 * ft_hifigan_resconv launches.  Unused arguments are ignored; an unknown field answers -1. */
int ft_voc_plan(int field, int a, int b, int c);

#ifdef __cplusplus
}
#endif
#endif /* FWDTACO_HIP_H */
