/* libmsn_hip.so -- C-ABI of the MI355X (gfx950) contrastive hot path.
 *
 * Drop-in boundary for the training step of ThomasHelfer/multimodal-supernovae:
 * encoders -> projection -> L2 normalise -> all-pairs similarity -> symmetric InfoNCE
 * -> backward -> RAdam.  The reference has no FFI of its own (it is pure PyTorch); each
 * entry point below replaces the stock-ATen op sequence of the cited reference lines
 * (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes binding a
 * reference maintainer would add.
 *
 * Conventions
 *  - the msn_set_* entry points are process-wide measurement / test switches (unsynchronised statics of the library): set them
 *    once, before work is enqueued, from the thread that enqueues it -- they are not thread-safe (INTEGRATION.md, round-4 notes);
 *    the data path keeps no mutable global state besides the mutex-protected arrival-counter slices of the work-list kernels;
 *  - every function returns 0 on success, MSN_ERR_SHAPE for a rejected argument (nothing
 *    is launched) or MSN_ERR_HIP for a failed launch; msn_last_error() gives the text;
 *  - all pointers are DEVICE pointers to fp32 unless stated (masks: 1 byte / element);
 *    matrices are row-major with explicit leading dimensions where strided use is allowed;
 *  - no allocation, no synchronisation: kernels are enqueued on `stream` (a hipStream_t);
 *    scratch memory is caller-owned (`ws`, sized by the matching *_workspace_bytes);
 *  - results are deterministic (no floating-point atomics anywhere).
 */
#ifndef MSN_HIP_H
#define MSN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSN_OK 0
#define MSN_ERR_SHAPE 1
#define MSN_ERR_HIP 2

typedef void* msn_stream_t; /* hipStream_t */

int msn_version(void);
const char* msn_last_error(void);
/* Measurement: one wave that stamps the shader-cycle and the 100-MHz real-time counters `microseconds` apart on `stream`:
 * out2[0] = shader cycles, out2[1] = real-time ticks (device memory) -> the clock the chip holds while whatever else runs meanwhile
 * (bench.py launches it on a side stream beside a training step: roofline.shader_clock_ghz). */
int msn_clock_probe(unsigned long long* out2, int microseconds, msn_stream_t stream);
/* number of visible HIP devices, or -1 when the HIP runtime cannot be initialised */
int msn_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Dense fp32 GEMM on the f32-input matrix cores (v_mfma_f32_32x32x2_f32, exact fp32).
 * Replaces nn.Linear / 1x1-conv / patch-conv forward and both of their backward products:
 *   src/transformer_utils.py:45-47,89 (q/k/v, unifyheads), :102-106 (ff), :251 (projection),
 *   src/models_multimodal.py:54-56,75,85-88 (ConvMixer convs / head), :853-856 (MLP), :277 etc.
 *
 *   C[M,N] = epilogue( opA(A)[M,K] . opB(B)[K,N] + bias[N] )
 *
 * opA = MSN_OP_N: A stored [M][lda>=K];  MSN_OP_T: A stored [K][lda>=M].
 * opB = MSN_OP_N: B stored [K][ldb>=N];  MSN_OP_T: B stored [N][ldb>=K].
 *   forward  y = x W^T + b : (N, T);   dgrad dx = dy W : (N, N);   wgrad dW = dy^T x : (T, N).
 * epilogue:
 *   MSN_EPI_NONE      C = acc + bias
 *   MSN_EPI_RELU      C = max(acc + bias, 0)
 *   MSN_EPI_GELU      C = gelu(acc + bias) (erf form); if aux != NULL also aux = gelu'(acc + bias)
 *   MSN_EPI_RELU_BWD  C = acc * (aux > 0)            (aux = forward ReLU output)
 *   MSN_EPI_GELU_BWD  C = acc * aux                  (aux = the gelu' saved by the forward epilogue)
 *   MSN_EPI_ADD       C = acc + bias + aux           (residual add)
 * bias may be NULL.  `ws` is only needed for opA = T (split-K wgrad; see workspace_bytes).
 */
#define MSN_OP_N 0
#define MSN_OP_T 1
#define MSN_EPI_NONE 0
#define MSN_EPI_RELU 1
#define MSN_EPI_GELU 2
#define MSN_EPI_RELU_BWD 3
#define MSN_EPI_GELU_BWD 4
#define MSN_EPI_ADD 5
/* precision of the inner products (inputs / outputs are fp32 in every mode):
 *   MSN_PREC_F32     exact fp32 on v_mfma_f32_32x32x2_f32 (default; 157 TFLOP/s peak)
 *   MSN_PREC_BF16X3  each operand split hi + lo into two bf16, three v_mfma_f32_32x32x16_bf16 products with
 *                    fp32 accumulation: ~1e-5 relative error per product, 5.3x the fp32 matrix rate
 *   MSN_PREC_BF16    operands rounded to bf16, one product (BASELINE cfg5 "bf16 on MFMA") */
#define MSN_PREC_F32 0
#define MSN_PREC_BF16X3 1
#define MSN_PREC_BF16 2

size_t msn_sgemm_workspace_bytes(int opA, int opB, int64_t M, int64_t N, int64_t K);
/* Two fp32 kernel families sit behind msn_sgemm.
 *   mode 0: register-staged global->LDS copies with a distance-1 prefetch; takes every shape.
 *   mode 3 (default): LDS-DMA pipeline (global_load_lds, no staging registers, no ds_write), 4 waves per
 *           workgroup, 2 x 32-deep K ring, two workgroups per CU.  Used where it applies (16-B aligned
 *           operands, K % 32 == 0); other shapes take mode 0.
 *   mode 1 / 2: LDS-DMA with 8 waves per workgroup and a 3 x 32 / 2 x 64 deep ring (one workgroup per CU).
 *   mode 4: persistent workgroups of 4 multiplying + 2 loader waves (the loaders issue the ring's LDS-DMA for the
 *           whole sequence of tiles, so epilogue stores never sit in front of an operand wait); 128-wide tiles only.
 *           Measured equal to mode 3 on long K and slower on K <= 384: kept as an alternative.
 * All modes give bit-identical results (same k order per accumulator).  Process-wide. */
int msn_set_gemm_variant(int mode);
/* Tail split (default on): a product whose 128 x 128 tiles do not fill a whole number of rounds of the chip's
 * 512 resident workgroups has the tiles of the last, partly filled round cut into K-slabs; msn_sgemm_workspace_bytes
 * covers the slabs.  enabled = 1 (default): the workgroup that stores a tile's last slab (device-scope arrival
 * counter in module memory, one slice per stream) sums the slabs in slab order and applies the epilogue inside the
 * same launch; 2: a finishing launch does (bit-identical: same order); 0: no slabs.  Results of the tail tiles
 * differ from the unsplit order in the last bits.  Process-wide. */
int msn_set_gemm_tail_split(int enabled);
/* Measurement switch: tile width of products with N > 64: 0 = planned (default), 64, 128. */
int msn_set_gemm_tile_n(int bn);
int msn_sgemm(int opA, int opB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
              const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, int epilogue,
              float* aux, int64_t ldaux, int precision, void* ws, size_t ws_bytes, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Work-list launch: up to 3 independent products in ONE persistent launch (gemm_list.hip).  The (tile, K-step) pairs
 * of all products form one sequence that is cut into equal ranges, one per resident workgroup; a tile cut by a range
 * boundary is finished by the last of its contributors to arrive (slabs of raw accumulators summed in k order:
 * deterministic).  Built for the 128 - 512 rows per GPU that strong scaling of the global batch leaves a rank, where a
 * single product cannot fill the chip's 512 workgroup slots, and for the two backward products of a Linear
 * (src/transformer_utils.py:45-47,89,102-106: dX = dY . W and dW = dY^T . X share dY and are independent) -- the weight
 * gradient needs no split count and no reduction launch.  `colsum` (opA = T only, may be NULL): also out[M] = column
 * sums of A, i.e. the bias gradient of the same Linear.  Products the kernel does not take (N or M <= 64, K % 32 != 0,
 * unaligned operands, precision != fp32) are issued one by one through msn_sgemm / msn_wgrad_bias -- same results as
 * calling those.  Against the one-by-one path the list kernel's results differ in the last bits (another k order).
 * msn_sgemm itself takes the list kernel for an opA = N product of at most 1024 128 x 128 tiles and K >= 1024 whose last round of
 * workgroups is under-filled (the balance gained outweighs the slabs of the cut tiles).
 * msn_set_gemm_list(mode): 1 = all of the above (default); 0 = no work-list launch at all (lists one by one; measurements, bit
 * comparisons); 2 = lists only, single products never; 3 = lists + every single product the kernel can take (tests).  Process-wide. */
typedef struct msn_gemm_desc {
    int opA, opB;
    int64_t M, N, K;
    const float* A;
    int64_t lda;
    const float* B;
    int64_t ldb;
    float* C;
    int64_t ldc;
    const float* bias;
    int epilogue;
    float* aux;
    int64_t ldaux;
    float* colsum;
} msn_gemm_desc;
size_t msn_sgemm_list_workspace_bytes(int n, const msn_gemm_desc* products);
int msn_sgemm_list(int n, const msn_gemm_desc* products, int precision, void* ws, size_t ws_bytes, msn_stream_t stream);
int msn_set_gemm_list(int mode);
/* Zero the arrival counters of the in-kernel tile finishes (tail split, work-list launch) of the current device: they
 * are zero between launches by construction, but a launch that faulted or was aborted half-way leaves them dirty. */
int msn_reset_gemm_counters(msn_stream_t stream);

/* Weight + bias gradient of a Linear in one launch (the backward of torch.nn.functional.linear as used at
 * ref src/transformer_utils.py:33-36, :103-107 and every nn.Linear of src/models_multimodal.py):
 *   dW[M x N] = dY^T X,   db[M] = column sums of dY,   dY: K x M (row stride lddy), X: K x N (row stride ldx).
 * On the LDS-DMA kernels the column sums ride on the A fragments the product already holds (no second pass over
 * dY); other shapes / precisions run msn_sgemm + msn_colsum.  Workspace: msn_wgrad_bias_workspace_bytes. */
size_t msn_wgrad_bias_workspace_bytes(int64_t M, int64_t N, int64_t K);
int msn_wgrad_bias(int64_t M, int64_t N, int64_t K, const float* dY, int64_t lddy, const float* X, int64_t ldx,
                   float* dW, int64_t lddw, float* db, int precision, void* ws, size_t ws_bytes,
                   msn_stream_t stream);

/* out[n] = sum_m X[m][n]  (bias gradients).  ws >= msn_colsum_workspace_bytes(M, N). */
size_t msn_colsum_workspace_bytes(int64_t M, int64_t N);
int msn_colsum(const float* X, int64_t ldx, int64_t M, int64_t N, float* out, void* ws, size_t ws_bytes,
               msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused symmetric InfoNCE ("clip_loss") for one modality pair -- src/loss.py:14-38.
 * The N x N logit matrix S = exp(log_scale) * E2 . E1^T + bias is never materialised.
 *
 * Row-sharded over ranks: this rank owns rows [q_offset, q_offset + b) of both modalities
 * (E1_loc (b1 x D), E2_loc (b2 x D)) and holds the all-gathered matrices E1_all (n1 x D),
 * E2_all (n2 x D).  Single process: *_loc == *_all, q_offset = 0.  n = min(n1, n2) (:31).
 *   fwd: lse_row[i] = LSE_j S[q_offset+i][j]   (b2 values; rows of S come from E2)
 *        lse_col[i] = LSE_j S[j][q_offset+i]   (b1 values; columns of S come from E1)
 *        loss[0]    = 1/(2n) * sum_{local i, q_offset+i < n} (lse_row + lse_col - 2 S_ii)
 *                     (this rank's share; the total loss is the sum over ranks)
 *   bwd: needs the LSE vectors of ALL rows (all-gathered: lse_row_all (n2), lse_col_all (n1))
 *        and the upstream gradient `grad_out` (device scalar).  Writes dE1_loc, dE2_loc (the
 *        complete gradient of the global loss w.r.t. the local rows -- no reduce-scatter) and
 *        dscale_dbias[2] = this rank's share of d/dlog_scale and d/dbias (sum over ranks).
 * log_scale, bias, grad_out are DEVICE scalars (no host synchronisation).  Embedding width (the reference takes any
 * enc_dim, src/models_multimodal.py:101): any 1 <= D <= 256 (tiles 8/16/32/64/128/256 columns wide, zero beyond column D),
 * and 256 < D <= 1024 with D a multiple of 32 (the waves of a workgroup split D); other widths are refused.  Rows of any
 * stride >= D, 4-byte aligned.
 */
size_t msn_infonce_workspace_bytes(int b1, int b2, int n1, int n2, int D);
int msn_infonce_fwd(const float* E1_loc, int64_t ld1, int b1, const float* E2_loc, int64_t ld2, int b2,
                    const float* E1_all, int64_t ld1a, int n1, const float* E2_all, int64_t ld2a, int n2,
                    int D, int q_offset, const float* log_scale, const float* bias, float* lse_row,
                    float* lse_col, float* loss, void* ws, size_t ws_bytes, msn_stream_t stream);
int msn_infonce_bwd(const float* E1_loc, int64_t ld1, int b1, const float* E2_loc, int64_t ld2, int b2,
                    const float* E1_all, int64_t ld1a, int n1, const float* E2_all, int64_t ld2a, int n2,
                    int D, int q_offset, const float* log_scale, const float* bias,
                    const float* lse_row_all, const float* lse_col_all, const float* grad_out,
                    float* dE1_loc, int64_t ldd1, float* dE2_loc, int64_t ldd2, float* dscale_dbias,
                    void* ws, size_t ws_bytes, msn_stream_t stream);

/* Label-aware (supervised) contrastive loss of one modality pair: SupCon (Khosla et al. 2020) in its cross-modal form, the
 * bidirectional loss of UniCL (Yang et al. 2022).  labels_all holds the int32 label of every gathered row (n of them); a
 * negative label is "class unknown" and makes the row a singleton class.  With S = exp(log_scale) * E2 . E1^T + bias,
 *   P_ij = [i == j] or (y_i == y_j and y_i >= 0),   c_i = sum_j P_ij >= 1,
 *   loss = 1/(2n) * sum_i [ LSE_j S_ij - (1/c_i) sum_j P_ij S_ij + LSE_j S_ji - (1/c_i) sum_j P_ji S_ji ]
 *   G_ij = dloss/dS_ij = ( softmax_row(S)_ij + softmax_col(S)_ij - 2 P_ij / c_i ) / (2n)
 *   dE2 = s G E1, dE1 = s G^T E2, dlog_scale = sum_ij G_ij (S_ij - bias), dbias = sum_ij G_ij.
 * With all labels distinct this is msn_infonce_*.  Same row-sharded calling convention as msn_infonce_*, with b1 == b2,
 * n1 == n2 and q_offset + b <= n (anything else is refused) and 1 <= D <= 256 (wider embeddings are not built).
 *   fwd: lse_row, lse_col (b values each) as msn_infonce_fwd; cnt[i] = c of local row i (b int32 values, exact);
 *        loss[0] = 1/(2n) * sum_{local i} (lse_row_i + lse_col_i - the two positive means): this rank's share.
 *   bwd: the LSE vectors of ALL rows, the counts of the LOCAL rows and grad_out (device scalar); writes dE1_loc, dE2_loc
 *        (complete for the local rows) and dscale_dbias[2] = this rank's share of (dlog_scale, dbias).
 * No atomics, no zeroed scratch, the same bits on every run, no host read.  Workspace: msn_supcon_workspace_bytes (0 for
 * a shape that is refused). */
size_t msn_supcon_workspace_bytes(int b1, int b2, int n1, int n2, int D);
int msn_supcon_fwd(const float* E1_loc, int64_t ld1, int b1, const float* E2_loc, int64_t ld2, int b2,
                   const float* E1_all, int64_t ld1a, int n1, const float* E2_all, int64_t ld2a, int n2, int D,
                   int q_offset, const int32_t* labels_all, const float* log_scale, const float* bias,
                   float* lse_row, float* lse_col, int32_t* cnt, float* loss, void* ws, size_t ws_bytes,
                   msn_stream_t stream);
int msn_supcon_bwd(const float* E1_loc, int64_t ld1, int b1, const float* E2_loc, int64_t ld2, int b2,
                   const float* E1_all, int64_t ld1a, int n1, const float* E2_all, int64_t ld2a, int n2, int D,
                   int q_offset, const int32_t* labels_all, const float* log_scale, const float* bias,
                   const float* lse_row_all, const float* lse_col_all, const int32_t* cnt, const float* grad_out,
                   float* dE1_loc, int64_t ldd1, float* dE2_loc, int64_t ldd2, float* dscale_dbias, void* ws,
                   size_t ws_bytes, msn_stream_t stream);

/* SigLIP-style loss with the reference's sign convention -- sigmoid_loss, src/loss.py:68-83:
 *   Z = -(E2 . E1^T) exp(log_scale) + bias (fp32);  loss = mean_ij softplus(z_ij Z_ij) evaluated in fp64,
 *   z = +1 on the diagonal, -1 elsewhere (mean over all n x n entries).  Same row-sharded calling
 *   convention, embedding widths and workspace as msn_infonce_*; both modalities have b local / n global rows.
 *   fwd writes this rank's share of the loss; bwd writes dE1_loc, dE2_loc and (dlog_scale, dbias) shares. */
int msn_sigmoid_loss_fwd(const float* E1_loc, int64_t ld1, const float* E2_loc, int64_t ld2, int b,
                         const float* E1_all, int64_t ld1a, const float* E2_all, int64_t ld2a, int n, int D,
                         int q_offset, const float* log_scale, const float* bias, float* loss, void* ws,
                         size_t ws_bytes, msn_stream_t stream);
int msn_sigmoid_loss_bwd(const float* E1_loc, int64_t ld1, const float* E2_loc, int64_t ld2, int b,
                         const float* E1_all, int64_t ld1a, const float* E2_all, int64_t ld2a, int n, int D,
                         int q_offset, const float* log_scale, const float* bias, const float* grad_out,
                         float* dE1_loc, int64_t ldd1, float* dE2_loc, int64_t ldd2, float* dscale_dbias,
                         void* ws, size_t ws_bytes, msn_stream_t stream);

/* Retrieval rank for the validation "AUC" -- get_ROC_data, src/utils.py:380-411: for unit-norm rows,
 * rank[i] = #{ j != i : <E2_i, E1_j> > <E2_i, E1_i> } (position of the true partner in row i's similarity
 * ranking; the reference sorts every row in a host loop).  Widths as msn_infonce_*: 1 <= D <= 256, or 256 < D <= 1024
 * with D a multiple of 32.  workspace: msn_infonce_workspace_bytes(n,n,n,n,D). */
int msn_retrieval_rank(const float* E1, int64_t ld1, const float* E2, int64_t ld2, int n, int D, int* rank,
                       void* ws, size_t ws_bytes, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension (rows x cols, cols % 4 == 0, cols <= 1024), eps inside the
 * square root -- nn.LayerNorm as used at src/transformer_utils.py:97-98,111,114 (post-norm; the
 * residual sum is produced by the preceding GEMM's MSN_EPI_ADD epilogue).
 * fwd writes y and the per-row mean / rstd; bwd consumes them and returns dx (+ `add`, the
 * gradient of a residual branch around the norm, when non-NULL), dgamma, dbeta.
 */
int msn_layernorm_fwd(const float* x, int64_t ldx, int64_t rows, int cols, const float* gamma,
                      const float* beta, float eps, float* y, int64_t ldy, float* mean, float* rstd,
                      msn_stream_t stream);
size_t msn_layernorm_bwd_workspace_bytes(int64_t rows, int cols);
int msn_layernorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t rows, int cols,
                      const float* mean, const float* rstd, const float* gamma, const float* add,
                      int64_t ldadd, float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws,
                      size_t ws_bytes, msn_stream_t stream);

/* y = x / ||x||_2 per row, NO epsilon (src/models_multimodal.py:279,286,293,304); inv_norm[r] = 1/||x_r||.
 * bwd: dx = inv_norm * (dy - y <y, dy>). */
int msn_l2norm_fwd(const float* x, int64_t ldx, int64_t rows, int cols, float* y, int64_t ldy,
                   float* inv_norm, msn_stream_t stream);
int msn_l2norm_bwd(const float* dy, int64_t lddy, const float* y, int64_t ldy, int64_t rows, int cols,
                   const float* inv_norm, float* dx, int64_t lddx, msn_stream_t stream);

/* Token embedding of an irregular time series -- src/transformer_utils.py:166-176 and :214-231:
 *   out[b,t,c] = x[b,t] * w[c] + bw[c] + (c even ? sin : cos)(t[b,t] * omega[c/2]) + band[t / (T/nband)][c]
 * omega[k] = exp(-2k ln(norm) / e) is passed in (e/2 floats); band (nband x e) only when nband > 1.
 * bwd returns dw, dbw (e each) and dband (nband x e; NULL when nband == 1); x, t get no gradient. */
int msn_time_embed_fwd(const float* x, const float* t, int64_t B, int T, int e, const float* w,
                       const float* bw, const float* omega, const float* band, int nband, float* out,
                       msn_stream_t stream);
size_t msn_time_embed_bwd_workspace_bytes(int64_t B, int e, int nband);
int msn_time_embed_bwd(const float* dy, const float* x, int64_t B, int T, int e, int nband, float* dw,
                       float* dbw, float* dband, void* ws, size_t ws_bytes, msn_stream_t stream);

/* Masked pooling over tokens -- src/transformer_utils.py:234-239.  mask: (B, T) bytes (torch.bool).
 * mode MSN_POOL_MEAN: sum_t x*mask / sum_t mask (writes count[b]; an all-false row gives NaN as
 * the reference does); MSN_POOL_MAX: max_t (x*mask) over ALL t (writes argmax (B, e) int32). */
#define MSN_POOL_MEAN 0
#define MSN_POOL_MAX 1
int msn_masked_pool_fwd(const float* x, const uint8_t* mask, int64_t B, int T, int e, int mode, float* out,
                        int* argmax, float* count, msn_stream_t stream);
int msn_masked_pool_bwd(const float* dout, const uint8_t* mask, int64_t B, int T, int e, int mode,
                        const int* argmax, const float* count, float* dx, msn_stream_t stream);
/* y[r,:] = x[r,:] * mask[r]  (the `x * mask[:, :, None]` of :235; its own backward) */
int msn_mask_tokens(const float* x, const uint8_t* mask, int64_t rows, int e, float* y, msn_stream_t stream);

/* dst[r][0..cols) += src[r][0..cols) for r < rows, both row-strided (cols, ldd, lds multiples of 4; 16-byte aligned).
 * The class-token read-out of the build-defined ViT: only token 0 of the last block feeds the head, so that block's
 * attention output / MLP run on the B class rows alone and their input gradient is added back into row 0 of every
 * sample of the dense (B, T, e) gradient (no reference counterpart: the ViT is build-defined). */
int msn_add_rows(float* dst, int64_t ldd, const float* src, int64_t lds, int64_t rows, int cols, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * fp32-GRADE products on the bf16 matrix cores from resident bf16 PLANES (pgemm.hip) -- the same nn.Linear products
 * msn_sgemm multiplies (ref src/transformer_utils.py:45-47, 89, 102-106, 251; src/models_multimodal.py:277), for the wide
 * layers of the build-defined ViT towers.  An fp32 matrix is kept in HBM as `planes` bf16 planes, x = p0 + p1 (+ p2) with
 * p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1): three planes hold an fp32 value EXACTLY (3 x 8 significand
 * bits, fp32 exponent range).  A product sums the plane products with pa + pb < planes on v_mfma_f32_32x32x16_bf16 with
 * fp32 accumulation: planes = 3 -> 6 MFMA products, terms dropped <= 2^-26 |a||b| (fp32 grade); planes = 2 -> 3 products,
 * dropped <= 2^-17 |a||b|.
 * Plane matrix of a logical R x C matrix ("blocked planes"): 32-row x 16-column blocks, block (rb, cb) = `planes`
 * consecutive 1-KB images [32][16] bf16; byte offset of (r, c, plane) = (((r / 32) * CB + c / 16) * planes + plane) * 1024
 * + (r % 32) * 32 + (c % 16) * 2, CB = 2 * ceil(C / 32); rows / columns past R / C are zero.  msn_plane_bytes gives its size.
 *   msn_plane_split:  fp32 (R x C, row stride ldx) -> plane matrix; transposed = 1 writes the planes of the C x R
 *                     transpose (weights for the input-gradient products).  colsum (nullable, untransposed only):
 *                     out[c] = sum_r x[r][c] (bias gradients); ws >= msn_plane_split_colsum_workspace_bytes.
 *   msn_plane_merge:  plane matrix -> fp32 (tests).
 *   msn_pgemm_nt:     C[M][N] = epilogue(A[M][K] . B[N][K]^T + bias); A, B plane matrices (M x K, N x K).  C is fp32
 *                     (row stride ldc) or, with c_planes = 1, the plane matrix of the M x N result (N % 16 == 0) -- the
 *                     operand of the next product, split in the epilogue.  Epilogues as msn_sgemm (MSN_EPI_*; aux fp32).
 *                     colsum_out (nullable): column sums of the values written to C; ws >= msn_pgemm_nt_colsum_workspace_bytes.
 *   msn_pgemm_tn:     C[N][K] (fp32) = sum_m A[m][N]^T . B[m][K] (weight gradient dY^T . X); A, B plane matrices with the
 *                     reduction on the rows (M x N, M x K); reduction split over workgroups, fixed-order slab sums;
 *                     ws >= msn_pgemm_tn_workspace_bytes.
 * Results are deterministic. */
size_t msn_plane_bytes(int64_t R, int64_t C, int planes);
size_t msn_plane_split_colsum_workspace_bytes(int64_t R, int64_t C);
int msn_plane_split(const float* x, int64_t ldx, int64_t R, int64_t C, int planes, int transposed, void* out, float* colsum,
                    void* ws, size_t ws_bytes, msn_stream_t stream);
/* msn_plane_split of several matrices in ONE launch (per 64 items): the weights of every block of a tower, or their
 * transposes.  items: host array; out of item i holds msn_plane_bytes(R, C, planes) bytes (transposed: of (C, R)). */
typedef struct msn_split_item {
    const float* x;
    int64_t ldx, R, C;
    int transposed;
    void* out;
} msn_split_item;
int msn_plane_split_list(int n, const msn_split_item* items, int planes, msn_stream_t stream);
int msn_plane_merge(const void* planes_in, int planes, int64_t R, int64_t C, float* y, int64_t ldy, msn_stream_t stream);
size_t msn_pgemm_nt_colsum_workspace_bytes(int64_t M, int N);
/* Workspace of msn_pgemm_nt: the column sums' partials (want_colsum) or the slabs of the TAIL split -- the tiles that do not
 * fill a round of the 256 persistent workgroups are cut into K-segments, one per workgroup, and a finishing launch sums
 * the segments in K order and applies the epilogue (fp32 outputs, epilogues NONE / RELU / ADD; deterministic).  Without a
 * workspace (NULL / too small) the tail tiles are multiplied whole.  msn_set_pgemm_tail_split(0) turns the split off. */
size_t msn_pgemm_nt_workspace_bytes(int64_t M, int N, int K, int planes, int c_planes, int epilogue, int want_colsum);
int msn_set_pgemm_tail_split(int enabled);
int msn_pgemm_nt(int64_t M, int N, int K, int planes, const void* A, const void* B, void* C, int64_t ldc, int c_planes,
                 const float* bias, int epilogue, float* aux, int64_t ldaux, float* colsum_out, void* ws, size_t ws_bytes,
                 msn_stream_t stream);
size_t msn_pgemm_tn_workspace_bytes(int64_t M, int N, int K, int planes);
int msn_pgemm_tn(int64_t M, int N, int K, int planes, const void* A, const void* B, float* C, int64_t ldc, void* ws,
                 size_t ws_bytes, msn_stream_t stream);
/* nn.LayerNorm as msn_layernorm_fwd / _bwd, writing the result as a plane matrix (the next product's operand): forward y
 * (y_planes; y fp32 optional, may be NULL), backward dx (fp32 AND planes; dx_colsum nullable = column sums of dx, the bias
 * gradient of the Linear below a residual add).  Workspace of the backward: msn_layernorm_bwd_workspace_bytes * 3 / 2. */
int msn_layernorm_fwd_planes(const float* x, int64_t ldx, int64_t rows, int cols, const float* gamma, const float* beta,
                             float eps, int planes, void* y_planes, float* y, int64_t ldy, float* mean, float* rstd,
                             msn_stream_t stream);
/* (With y == NULL and 260..400 columns, from 32 768 rows on, both directions take whole 32-row blocks per workgroup and write each
 * block's plane images as contiguous memory; y, dx and every plane byte are the same as the row-at-a-time kernels', the backward's
 * dgamma / dbeta / dx_colsum the same terms summed in another fixed order.) */
int msn_layernorm_bwd_planes(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t rows, int cols,
                             const float* mean, const float* rstd, const float* gamma, const float* add, int64_t ldadd,
                             float* dx, int64_t lddx, int planes, void* dx_planes, float* dgamma, float* dbeta,
                             float* dx_colsum, void* ws, size_t ws_bytes, msn_stream_t stream);
/* Self-attention forward over a packed qkv matrix (rows = (sample, token), columns q | k | v; ref src/transformer_utils.py:36-89)
 * whose output is written twice by the one kernel: `out` (fp32, (B T) x (H head_dim), row stride ldo -- the backward reads it) and
 * `out_planes` (msn_plane_bytes(B T, H head_dim, planes) bytes, 16-byte aligned): the operand of the output projection, bit for bit
 * what msn_plane_split(out) would write.  T <= 128 tokens, head_dim in {16, 32, 48, 64}, 16-byte aligned rows with strides % 4 == 0;
 * lse as msn_attention_fwd ([B][H][T][2]).  MSN_ERR_SHAPE otherwise (the caller runs msn_attention_fwd + msn_plane_split). */
int msn_attention_fwd_planes(const float* qkv, int64_t ldqkv, const uint8_t* key_mask, int B, int H, int T, int head_dim,
                             float scale, float* out, int64_t ldo, float* lse, int planes, void* out_planes, msn_stream_t stream);
/* Backward of the ViT blocks' self-attention (msn_attention_bwd on the packed q | k | v matrix of msn_pgemm_nt's qkv
 * product: qkv (B T x ldqkv >= 3 H hd), out / dout (B T x H hd), lse as msn_attention_fwd wrote it), writing the gradient
 * dqkv (B T x 3 H hd) as a PLANE matrix -- the operand of the two products that consume it -- and, colsum_out non-NULL,
 * its column sums (the bias gradient of the qkv projection; workspace msn_attention_bwd_planes_workspace_bytes).  One
 * launch, one pass over the operands (see msn_set_attention_fused).  T <= 128, hd in {16, 32, 48, 64}, key_mask (B, T)
 * bytes or NULL.  Replaces msn_attention_bwd + msn_plane_split for the build-defined ViT (no reference counterpart:
 * the reference's image ViT is torch's nn.MultiheadAttention inside its build-defined encoder). */
size_t msn_attention_bwd_planes_workspace_bytes(int B, int H, int head_dim);
int msn_attention_bwd_planes(const float* qkv, int64_t ldqkv, const uint8_t* key_mask, int B, int H, int T, int head_dim,
                             float scale, const float* out, int64_t ldo, const float* lse, const float* dout, int64_t ldd,
                             int planes, void* dqkv_planes, float* colsum_out, void* ws, size_t ws_bytes,
                             msn_stream_t stream);
/* ---- the same products from TWO fp16 planes per operand (3 MFMA products instead of 6): x 2^e = h0 + h1 carries 22 significand
 * bits (bf16 planes: 8 per plane, so fp32 grade takes three), at half the matrix work.  fp16's exponent range is what this
 * costs: every plane matrix has a power-of-two scale chosen from its largest magnitude (msn_plane_split_f16 makes a pass for
 * it: m 2^e in [2^13, 2^14)); `scale` is two device floats: [0] = 2^-e, which the products multiply into their sums (exact),
 * [1] = the bits of m.  reuse_scale = 1 splits with the scale already in `scale` (a weight matrix and its transpose share one).
 * Products: v_mfma_f32_32x32x16_f16, two accumulator sets, K chunks as msn_pgemm_nt; fp32 results only.  Measured against fp64
 * (tests/test_pgemm_gpu.py::test_fp32_grade_gate_*[f16x3-*]): 0.3 - 0.6 x the native fp32 kernel's error on normal, wide-range,
 * tiny and huge data, but 2.2 - 2.7 x on cancellation-heavy data (22-bit operands) -- NOT fp32 grade by the 1.5 x gate, so an
 * opt-in of this interface only; 1.4 - 1.6 x the rate of the six-product form (profiles/r04_pgemm_f16.txt).  Layout of the
 * plane matrix: as msn_plane_split with planes = 2. */
int msn_plane_split_f16(const float* x, int64_t ldx, int64_t R, int64_t C, int transposed, void* out, float* scale,
                        int reuse_scale, float* colsum, void* ws, size_t ws_bytes, msn_stream_t stream);
int msn_pgemm_nt_f16(int64_t M, int N, int K, const void* A, const float* scaleA, const void* B, const float* scaleB, float* C,
                     int64_t ldc, const float* bias, int epilogue, float* aux, int64_t ldaux, float* colsum_out, void* ws,
                     size_t ws_bytes, msn_stream_t stream);   /* workspace: msn_pgemm_nt_workspace_bytes(.., planes 2, ..) */
int msn_pgemm_tn_f16(int64_t M, int N, int K, const void* A, const float* scaleA, const void* B, const float* scaleB, float* C,
                     int64_t ldc, void* ws, size_t ws_bytes, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The feed-forward half of the reference's TransformerBlock for the NARROW towers -- z = x + Linear(4e -> e)(ReLU(Linear(e -> 4e)(x))),
 * ref src/transformer_utils.py:102-106, 114; emb 32 / hidden 128 (the spectrum transformer) -- as ONE kernel per direction whose
 * 4e-wide hidden activations never reach HBM (csrc/ffn_planes.hip): fp32-grade arithmetic on the bf16 matrix cores (three planes per
 * operand, six products, as msn_pgemm_*), both weights resident in LDS as the plane matrices msn_plane_split writes:
 *   w1_planes  = planes of ff.0.weight [4e][e];  w2t_planes = planes of ff.2.weight TRANSPOSED [4e][e] (msn_plane_split, transposed = 1).
 *   msn_ffn_fwd:  z[M][e] = x + relu(x W1^T + c1) W2^T + c2.
 *   msn_ffn_bwd:  dx = dz + ((dz W2) o (pre > 0)) W1 (the hidden tile is RECOMPUTED with the forward's instructions: the same bits, no
 *                 mask is stored), dw1 [4e][e], dc1 [4e], dw2 [e][4e], dc2 [e] (per-workgroup partials in ws, summed in a fixed order
 *                 by a finishing launch: deterministic); ws >= msn_ffn_bwd_workspace_bytes.
 * msn_ffn_supported(M, emb, hidden): the shapes this build takes (emb 32, hidden 128); every other block keeps msn_sgemm. */
int msn_ffn_supported(int64_t M, int emb, int hidden);
int msn_ffn_fwd(const float* x, int64_t ldx, int64_t M, int emb, int hidden, const void* w1_planes, const void* w2t_planes,
                const float* c1, const float* c2, float* z, int64_t ldz, msn_stream_t stream);
size_t msn_ffn_bwd_workspace_bytes(int64_t M, int emb, int hidden);
int msn_ffn_bwd(const float* x, int64_t ldx, const float* dz, int64_t lddz, int64_t M, int emb, int hidden, const void* w1_planes,
                const void* w2t_planes, const float* c1, float* dx, int64_t lddx, float* dw1, float* dc1, float* dw2, float* dc2,
                void* ws, size_t ws_bytes, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * bf16-RESIDENT products for BASELINE.json configs[4] (ViT-B/16 "bf16 on MFMA"; build-defined encoder, no reference
 * counterpart -- the reference has no mixed precision): operands are bf16 in HBM (uint16 bit patterns), accumulation fp32.
 *   msn_bgemm_nt:  C[M][N] = epi(A[M][K] . B[N][K]^T + bias); K % 64 == 0, N % 4 == 0, 16-byte aligned rows.
 *                  epilogue 0 none (C fp32 or bf16), 1 GELU (aux <- bf16 pre-activation, C <- bf16 gelu), 2 GELU' (C <-
 *                  acc * gelu'(aux bf16); C fp32 or bf16), 3 ADD (C fp32 <- acc + bias + aux fp32).
 *   msn_bgemm_tn:  C[N][K] (fp32) = sum_m A[m][N]^T . B[m][K]  (weight gradient dY^T . X), reduction split over m with
 *                  fixed-order slab sums; ws >= msn_bgemm_tn_workspace_bytes.
 *   msn_cast_bf16 / msn_cast_bf16_transposed: y = bf16(x) (n % 8 == 0) / y[c][r] = bf16(x[r][c]).
 *   msn_bcolsum:   out[n] = sum_m X[m][n] for bf16 X (bias gradients).
 *   msn_layernorm_fwd_bf16 / msn_layernorm_bwd_bf16: nn.LayerNorm as msn_layernorm_fwd / _bwd, writing y as bf16 /
 *                  writing a bf16 copy of dx next to the fp32 one. */
int msn_bgemm_nt(int64_t M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                 int c_bf16, const float* bias, int epilogue, void* aux, int64_t ldaux, float* colsum_out, void* ws,
                 size_t ws_bytes, msn_stream_t stream);
  /* one persistent workgroup per CU walks the 256 x 256 tiles and keeps its LDS ring of K-tiles running across tile boundaries (one
     workgroup per tile below 257 tiles).  colsum_out (nullable): out[n] = sum_m C[m][n] from the epilogue (the
                 bias gradient of the Linear whose output gradient C is); ws >= msn_bgemm_nt_colsum_workspace_bytes(M, N) */
size_t msn_bgemm_nt_colsum_workspace_bytes(int64_t M, int N);
size_t msn_bgemm_tn_workspace_bytes(int64_t M, int N, int K);
int msn_bgemm_tn(int64_t M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc,
                 void* ws, size_t ws_bytes, msn_stream_t stream);
int msn_cast_bf16(const float* x, int64_t n, void* y, msn_stream_t stream);
int msn_cast_bf16_transposed(const float* x, int R, int C, void* y, msn_stream_t stream);
/* msn_cast_bf16 / msn_cast_bf16_transposed of a LIST of contiguous (R, C) fp32 matrices in ONE launch (the bf16-resident trunk: four
 * weights per block forward, four transposed copies backward): y (R, C) or, transposed != 0, (C, R), bf16, round to nearest even. */
typedef struct msn_cast_item {
    const float* x;
    int64_t R, C;
    int transposed;
    void* y;
} msn_cast_item;
int msn_cast_bf16_list(int n, const msn_cast_item* items, msn_stream_t stream);
size_t msn_bcolsum_workspace_bytes(int64_t M, int N);
int msn_bcolsum(const void* X, int64_t ldx, int64_t M, int N, float* out, void* ws, size_t ws_bytes, msn_stream_t stream);
int msn_layernorm_fwd_bf16(const float* x, int64_t ldx, int64_t rows, int cols, const float* gamma, const float* beta,
                           float eps, void* y_bf16, int64_t ldy, float* mean, float* rstd, msn_stream_t stream);
/* Self-attention on the bf16 matrix cores, 64-wide heads, T <= 256 tokens, no key mask (the cfg5 ViT-B/16 attention;
 * build-defined, scale 1/sqrt(head_dim)): qkv is the (B*T, ld >= 3*H*64) bf16 matrix [q | k | v] the packed projection
 * writes, out / dout (B*T, H*64) bf16, lse (B, H, T) fp32; bwd writes dqkv in qkv's layout (bf16); delta = (B, H, T) scratch. */
int msn_attention_bf16_fwd(const void* qkv, int64_t ld, int B, int H, int T, float scale, void* out, int64_t ldo, float* lse,
                           msn_stream_t stream);
int msn_attention_bf16_bwd(const void* qkv, int64_t ld, const void* out, int64_t ldo, const void* dout, int64_t ldd,
                           const float* lse, int B, int H, int T, float scale, void* dqkv, float* delta, float* colsum_out,
                           float* colsum_ws, msn_stream_t stream);   /* colsum_out (3*H*64, nullable): column sums of dqkv = the
                           bias gradient of the packed projection; colsum_ws: B x 3*H*64 floats */
int msn_layernorm_bwd_bf16(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t rows, int cols,
                           const float* mean, const float* rstd, const float* gamma, const float* add, int64_t ldadd,
                           float* dx, int64_t lddx, void* dx_bf16, float* dgamma, float* dbeta, float* dx_colsum, int dy_is_bf16,
                           void* ws, size_t ws_bytes, msn_stream_t stream);   /* dx_colsum (nullable): column sums of dx = the bias
                           gradient of the Linear feeding this LayerNorm's residual add; ws >= 1.5 x msn_layernorm_bwd_workspace_bytes
                           then.  dy_is_bf16: dy points at bf16 values, lddy in bf16 elements (the input-gradient product of cfg5
                           writes its result as bf16: half the bytes out of the GEMM epilogue and into this kernel) */

/* ------------------------------------------------------------------------------------------
 * Fused multi-head attention, exact fp32, no T x T tensor in memory -- SelfAttention.forward,
 * src/transformer_utils.py:36-89 (scale = 1/sqrt(emb); key-padding scores REPLACED by -1e7), also
 * the 1-query nn.MultiheadAttention pooling (:240-246) and the build-defined ViT blocks.
 * q: (B, Tq, H*hd) rows `ldq` apart, batches `q_bstride` apart (0 = one query shared by the batch);
 * k, v: (B, Tk, H*hd); head h lives in columns h*hd .. h*hd+hd-1 (so a packed q|k|v buffer works by
 * pointer offset + ld = 3*H*hd).  key_mask: (B, Tk) bytes or NULL.  hd <= 512: up to 32 any width,
 * above 32 a multiple of 4 on 16-byte aligned rows (MSN_ERR_SHAPE otherwise; ops pads such heads with
 * zero columns); 132 .. 512 run on their own kernels (attention_wide.hip: the head dimension split over
 * the waves of a workgroup, keys / queries streamed through LDS in 16-row chunks), under every
 * msn_set_attention_path mode; hd > 512 is MSN_ERR_SHAPE.
 * lse: (B, H, Tq, 2) = (row max, log of the exp-sum), kept apart because a fully padded sample has
 * max = -1e7 where fp32 cannot hold the sum.  bwd recomputes the probabilities from lse; `delta` is
 * (B, H, Tq) scratch.
 */
int msn_attention_fwd(const float* q, int64_t ldq, int64_t q_bstride, const float* k, int64_t ldk,
                      int64_t k_bstride, const float* v, int64_t ldv, int64_t v_bstride,
                      const uint8_t* key_mask, int B, int H, int Tq, int Tk, int head_dim, float scale,
                      float* out, int64_t ldo, int64_t o_bstride, float* lse, msn_stream_t stream);
int msn_attention_bwd(const float* q, int64_t ldq, int64_t q_bstride, const float* k, int64_t ldk,
                      int64_t k_bstride, const float* v, int64_t ldv, int64_t v_bstride,
                      const uint8_t* key_mask, int B, int H, int Tq, int Tk, int head_dim, float scale,
                      const float* out, int64_t ldo, int64_t o_bstride, const float* lse,
                      const float* dout, int64_t ldd, int64_t d_bstride, float* delta, float* dq,
                      int64_t lddq, int64_t dq_bstride, float* dk, int64_t lddk, int64_t dk_bstride,
                      float* dv, int64_t lddv, int64_t dv_bstride, msn_stream_t stream);
/* Attention of ONE query per (sample, head) over T keys: the class-token row of the LAST block of the build-defined ViT (the head
 * reads token 0 only; the arithmetic is SelfAttention of ref src/transformer_utils.py:36-89 for a single query, no mask).
 * q / out / dout / dq: (B, H * 64) fp32 rows; kv / dkv: (B * T, >= 2 * H * 64) rows, keys in columns [0, H 64), values in
 * [H 64, 2 H 64), fp32 (kv_bf16 = 0) or bf16 (1: the bf16-resident tower; dkv is written in the same type, round to nearest
 * even); probs: (B, H, T) fp32, written by the forward and read by the backward.  A wave per pair, eight lanes on a key's 64
 * columns, every K and V row read once per direction (csrc/cls_attention.hip).  head_dim must be 64 and T <= 256
 * (msn_cls_attention_supported); every row 16-byte aligned.  Everything else stays with msn_attention_fwd / _bwd, which run this
 * shape as a 16-row query tile with fifteen rows of padding. */
int msn_cls_attention_supported(int T, int head_dim);
int msn_cls_attention_fwd(const float* q, int64_t ldq, const void* kv, int64_t ldkv, int kv_bf16, int B, int H, int T, int head_dim,
                          float scale, float* out, int64_t ldo, float* probs, msn_stream_t stream);
int msn_cls_attention_bwd(const float* q, int64_t ldq, const void* kv, int64_t ldkv, int kv_bf16, int B, int H, int T, int head_dim,
                          float scale, const float* out, int64_t ldo, const float* probs, const float* dout, int64_t ldd, float* dq,
                          int64_t lddq, void* dkv, int64_t lddkv, msn_stream_t stream);
/* The same class-token attention WITHOUT keys and values (csrc/cls_pool.hip).  With one query per (sample, head) the key | value
 * projection of every token folds into B-row products: score s[b,j,h] = scale (qt[b,h] . h1[b,j] + q[b,h] . bk_h) with
 * qt[b,h] = Wk_h^T q[b,h], and the attention row a[b,h] = Wv_h m[b,h] + bv_h with m[b,h] = sum_j p[b,j,h] h1[b,j], h1 = LN1(x).
 * What runs over every token is three streaming kernels, one workgroup per sample, a wave per token row:
 *   fwd: reads x (B*T rows of e floats, row stride ldx) once; LayerNorm per row with msn_layernorm_fwd's arithmetic (h1 is never
 *        stored); writes mean / rstd (B*T), the probabilities probs (B, H, T) and m (B, H, e).  qt: (B, H, e).  q (B rows, stride
 *        ldq) and bk (e) give the per-(b, h) score constant; both NULL = 0 (it cancels in the softmax).
 *   dqt: first half of the backward.  Reads x once, recomputes h1, and from dm[b,h] = Wv_h^T da[b,h] (B, H, e) and the forward's
 *        m forms ds[b,h,j] = p (dm . h1 - dm . m) (B, H, T) and dqt[b,h] = scale sum_j ds h1[b,j] (B, H, e).
 *   bwd: second half.  Reads x once more; dh1[b,j] = sum_h (p dm + scale ds qt), on the class row + dcls[b] (B rows, stride ldcls,
 *        nullable: the gradient that reaches h1 through the query, dq Wq with dq = Wk_h dqt -- it depends on dqt, which is why
 *        the backward is two launches with B-row products between them); LayerNorm backward of each dh1 row with
 *        msn_layernorm_bwd's arithmetic, + dskip[b] (nullable: the skip connection) on the class row; dx (row stride lddx) is
 *        written once.  dgamma / dbeta: per-workgroup partials in ws, summed in a fixed order (no atomics: two runs give the
 *        same bits).
 * Supported (msn_cls_pool_supported): e % 4 == 0, e <= 512, heads <= 8 dividing e, 1 <= T <= 256. */
int msn_cls_pool_supported(int T, int e, int heads);
int msn_cls_pool_fwd(const float* x, int64_t ldx, int B, int T, int e, int heads, const float* gamma, const float* beta, float eps,
                     const float* qt, const float* q, int64_t ldq, const float* bk, float scale, float* mean, float* rstd,
                     float* probs, float* m, msn_stream_t stream);
int msn_cls_pool_dqt(const float* x, int64_t ldx, int B, int T, int e, int heads, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, const float* probs, const float* m, const float* dm, float scale,
                     float* ds, float* dqt, msn_stream_t stream);
size_t msn_cls_pool_bwd_workspace_bytes(int B, int e);
int msn_cls_pool_bwd(const float* x, int64_t ldx, int B, int T, int e, int heads, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, const float* qt, const float* probs, const float* dm, const float* ds,
                     float scale, const float* dcls, int64_t ldcls, const float* dskip, int64_t ldskip, float* dx, int64_t lddx,
                     float* dgamma, float* dbeta, void* ws, size_t ws_bytes, msn_stream_t stream);
/* Two implementations sit behind msn_attention_*: vector-ALU kernels (head widths up to 32, any length; the
 * reference-native 8-wide heads, widths that are not a multiple of 4, unaligned operands) and matrix-core
 * kernels (v_mfma_f32_16x16x4_f32; any length -- chunked beyond 128 tokens; every head width that is a
 * multiple of 4 up to 128, run as the next multiple of 16 with zero columns: the ViT towers, the
 * reference's 16-wide spectrum heads -- beyond 128 tokens on the bf16 planes, msn_set_attention_planes --
 * and its default 128-wide heads (emb 256 / 2 heads)).  A head WIDER THAN 32 must be a multiple of 4 on
 * 16-byte aligned rows (MSN_ERR_SHAPE otherwise: pad the heads with zero columns -- the Python binding does;
 * the 64- / 128-wide vector-ALU instantiations of rounds 1-4 spilled up to 2 KB per lane and are gone).
 * mode 0 = automatic (default: matrix cores for widths >= 16 where they apply), 1 = vector-ALU wherever it
 * exists (widths up to 32), 2 = matrix cores whenever applicable, narrow heads included (measured no faster
 * there).  Process-wide; meant for tests. */
int msn_set_attention_path(int mode);
/* Self-attention backward over up to 128 tokens with heads up to 64 wide (the ViT towers): 1 (default) = ONE launch that
 * holds Q, K, V and dO of a (sample, head) in LDS together -- one pass over the operands, delta never in memory; 0 = the
 * dQ kernel followed by the dK,dV kernel (same products in the same order); 3 = the one-pass kernel without the shared
 * recomputation (up to 4 full tiles -- the ViT towers -- the default computes every score tile ONCE for dQ, dK and dV: the dQ
 * parts of the four key-tile waves meet in LDS; 80 instead of 112 MFMAs per tile pair).  Process-wide; measurements and tests. */
int msn_set_attention_fused(int on);
/* Sequences of more than 128 tokens with heads up to 16 wide (the reference's spectrum transformer on 1024-bin spectra /
 * 220-step series: emb 32, 2 heads -- src/transformer_utils.py:36-89): fp32-GRADE attention on the bf16 matrix cores
 * (csrc/attention_planes.hip).  Q, K, V, dO are split into three bf16 planes as they are staged into LDS (exact: three 8-bit
 * pieces of the fp32 significand), probabilities and score gradients are split in registers, and every product is the six
 * plane products of the plane GEMMs (v_mfma_f32_16x16x32_bf16; the head-dimension products pack two planes into one
 * instruction's 32 k).  Same arguments, statistics layout and results (to fp32 rounding) as the exact-fp32 matrix-core
 * kernels it replaces; the accuracy gate is tests/test_attention_planes_gpu.py (error against fp64 <= 1.5 x theirs).
 * The backward is ONE pass for 256 or more (sample, head) pairs -- every score tile computed once, dS transposed through LDS for
 * the dQ product, a workgroup per pair walking all key blocks and summing dq over them in place (a small launch computes
 * delta = rowsum(dO o O) first) -- and the dQ kernel followed by the dK,dV kernel below that.
 * mode: 0 = off (the v_mfma_f32_16x16x4_f32 kernels), 1 = on (default), 3 = on with the two-kernel backward everywhere, 5 = on
 * with the one-pass backward everywhere (tests, A/B runs).  Heads narrower than 16 take this path only under
 * msn_set_attention_path(2) (measured equal to the vector-ALU kernels there).
 * Process-wide, not thread-safe (as every msn_set_* switch). */
int msn_set_attention_planes(int mode);

/* ------------------------------------------------------------------------------------------
 * ConvMixer image tower pieces -- src/models_multimodal.py:38-95, channels-last token matrices
 * X[(b, i, j)][c].  The patch conv (stride = kernel = p, no bias, :54-56) and the 1x1 convs (:75)
 * are msn_sgemm on these matrices with the GELU epilogue.
 */
/* img (B, C, H, W) -> patches [(b, i, j)][(c, u, v)], grid = floor(H/p) x floor(W/p) (extra pixels unused) */
int msn_patchify(const float* img, int B, int C, int H, int W, int p, float* patches, msn_stream_t stream);
/* its adjoint: d img from d patches (zeros outside the grid) */
int msn_unpatchify(const float* dpatches, int B, int C, int H, int W, int p, float* dimg, msn_stream_t stream);

/* nn.BatchNorm2d over the rows of x (rows x C), :58,70,77.  training != 0: two-pass batch statistics,
 * `mean` / `rstd` (C each) written, running_mean / running_var updated in place when non-NULL
 * (momentum; unbiased variance) ; training == 0: running statistics are used.  y = bn(x) (+ residual),
 * then ReLU when relu != 0 (build-defined ResNet blocks).
 * bwd: dx = dL/dx, additionally multiplied by dact[.] when dact != NULL (conv -> GELU -> BN order:
 * dact is the gelu' that msn_sgemm's GELU epilogue / msn_dwconv_gelu_fwd saved). */
size_t msn_bn_workspace_bytes(int64_t rows, int C);
int msn_batchnorm_fwd(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                      int training, float momentum, float* running_mean, float* running_var,
                      const float* residual, int relu, float* y, float* mean, float* rstd, void* ws,
                      size_t ws_bytes, msn_stream_t stream);
/* dmasked = dy * (y > 0): gradient through a trailing ReLU (relu != 0 above), given its output y */
int msn_relu_mask(const float* dy, const float* y, int64_t total, float* dmasked, msn_stream_t stream);
int msn_batchnorm_bwd(const float* dy, const float* x, const float* dact, int64_t rows, int C,
                      const float* mean, const float* rstd, const float* gamma, int training, float* dx,
                      float* dgamma, float* dbeta, void* ws, size_t ws_bytes, msn_stream_t stream);
/* The same for BatchNorm + ReLU (y = relu(bn(x)) saved): dy is masked by y > 0 inside both passes. */
int msn_batchnorm_relu_bwd(const float* dy, const float* y, const float* x, int64_t rows, int C, const float* mean,
                           const float* rstd, const float* gamma, int training, float* dx, float* dgamma, float* dbeta,
                           void* ws, size_t ws_bytes, msn_stream_t stream);

/* Synchronised BatchNorm for data-parallel replicas (per-replica statistics differ from the
 * single-process statistics at the global batch).  The same two-pass statistics as msn_batchnorm_fwd / _bwd, cut at
 * the points where the CALLER all-reduces (SUM, RCCL) C floats (forward, twice) or 2C floats (backward):
 *   fwd: colsum(center = NULL) -> all-reduce -> mean_from_sum(count = global rows)
 *        -> colsum(center = mean) -> all-reduce -> rstd_from_sqdev (running statistics from the global batch)
 *        -> msn_batchnorm_apply
 *   bwd: bwd_sums (sums[0..C) = sum dy = the LOCAL d beta, sums[C..2C) = sum dy * xhat = the LOCAL d gamma; parameter
 *        gradients stay local sums, the gradient all-reduce adds the other ranks) -> all-reduce of a copy
 *        -> bwd_apply with the global sums and count. */
int msn_bn_colsum(const float* x, int64_t rows, int C, const float* center, float* out, void* ws, size_t ws_bytes,
                  msn_stream_t stream);
int msn_bn_mean_from_sum(const float* sum, int64_t count, int C, float* mean, msn_stream_t stream);
int msn_bn_rstd_from_sqdev(const float* sqdev, int64_t count, int C, float eps, float momentum, const float* mean,
                           float* running_mean, float* running_var, float* rstd, msn_stream_t stream);
int msn_batchnorm_apply(const float* x, int64_t rows, int C, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, const float* residual, int relu, float* y,
                        msn_stream_t stream);
int msn_bn_bwd_sums(const float* dy, const float* x, int64_t rows, int C, const float* mean, const float* rstd,
                    float* sums, void* ws, size_t ws_bytes, msn_stream_t stream);
int msn_bn_bwd_apply(const float* dy, const float* x, const float* dact, int64_t rows, int64_t count, int C,
                     const float* mean, const float* rstd, const float* gamma, const float* sums, float* dx,
                     msn_stream_t stream);

/* depthwise k x k conv, padding='same', + bias, + GELU (:65-69): x (B, gh, gw, C) channels-last,
 * w (C, 1, k, k).  fwd writes act = gelu(pre) and dact = gelu'(pre) with pre = conv + bias.
 * bwd: dx = conv^T(dpre) (+ add), dw (C,1,k,k), dbias (C; may be NULL). */
int msn_dwconv_gelu_fwd(const float* x, const float* w, const float* bias, int B, int gh, int gw, int C,
                        int k, float* dact, float* act, msn_stream_t stream);
size_t msn_dwconv_bwd_workspace_bytes(int B, int C, int k);
int msn_dwconv_bwd(const float* dpre, const float* x, const float* w, int B, int gh, int gw, int C, int k,
                   const float* add, float* dx, float* dw, float* dbias, void* ws, size_t ws_bytes,
                   msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused multi-tensor RAdam step (csrc/optim_steps.hip) with torch.optim.RAdam semantics (betas, eps, coupled L2 weight
 * decay, rectification once rho_t > 5) -- the optimiser of src/models_multimodal.py:306-310.
 * table: DEVICE array of n_tensors records of five 64-bit words {p*, g*, m*, v*, numel};
 * step is the 1-based update count.  One launch for the whole model; 28 B of HBM traffic / parameter.
 * beta1 / beta2 are doubles, as torch holds them: 1 / (1 - beta1^t) and the rectification term are derived from the exact
 * values, and the kernel receives beta and 1 - beta each rounded to float once (it never forms 1.f - beta).
 */
int msn_radam_step(const void* table, int n_tensors, int64_t max_numel, float lr, double beta1, double beta2,
                   float eps, float weight_decay, int64_t step, msn_stream_t stream);
/* The same step for a training step recorded in a HIP graph.  hyper: DEVICE block of 64 bytes, 8-byte aligned:
 *   bytes  0 .. 15  double beta1, beta2 (exact)
 *   bytes 16 .. 43  float lr, beta1, beta2, eps, weight_decay, 1 - beta1, 1 - beta2 (each rounded once from double by the host)
 *   bytes 44 .. 51  float inv_c1, rect_scale (written by every launch);  bytes 52 .. 63 padding
 * step_counter[1] (device int64: steps taken so far).  Every launch increments the counter and derives
 * 1 / (1 - beta1^t) and the rectification term from the exact betas ON the device, so replays need no host write; a changed
 * hyper-parameter is carried in by rewriting bytes 0 .. 43 on the replaying stream between two replays. */
int msn_radam_step_dev(const void* table, int n_tensors, int64_t max_numel, void* hyper, long long* step_counter,
                       msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused multi-tensor Adam / AdamW step: torch.optim's _single_tensor_adam (no amsgrad, not capturable) with every scalar
 * rounded to float once from the double given here.  table: DEVICE array of n_tensors (1 .. 65535) records of five 64-bit
 * words {p*, g*, m*, v*, numel}; step is the 1-based update count; 28 B of HBM traffic / parameter.  Per element:
 *   decoupled == 0 (Adam):   if (weight_decay != 0) grad = grad.add(param, alpha=weight_decay)     g = fma(wd, p, g)
 *   decoupled != 0 (AdamW):  param.mul_(1 - lr * weight_decay)                                     p = p * (float)(1 - lr*wd)
 *   exp_avg.lerp_(grad, 1 - beta1)                                                 m = fma(1 - beta1, g - m, m)   [1 - beta1 < 0.5;
 *                                                                                  else fma(-(1 - (1 - beta1)), g - m, g), as lerp_]
 *   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)                   v = fma(beta2, v, ((1 - beta2) * g) * g)
 *   denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)                  denom = sqrtf(v) / bc2_sqrt + eps
 *   param.addcdiv_(exp_avg, denom, value=-step_size)                               p = fma(-step_size, m / denom, p)
 * with step_size = (float)(lr / (1 - beta1^t)) and bc2_sqrt = (float)sqrt(1 - beta2^t) formed in double. */
int msn_adam_step(const void* table, int n_tensors, int64_t max_numel, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int decoupled, int64_t step, msn_stream_t stream);
/* The same step for a training step recorded in a HIP graph.  hyper: DEVICE block of 64 bytes, 8-byte aligned:
 *   bytes  0 .. 31  double lr, beta1, beta2, weight_decay (exact)
 *   bytes 32 .. 47  float beta2, eps, 1 - beta1, 1 - beta2 (each rounded once from double by the host)
 *   bytes 48 .. 59  float step_size, bc2_sqrt, wd_term (written by every launch; wd_term = weight_decay, or for
 *                   decoupled != 0 the factor 1 - lr * weight_decay);  bytes 60 .. 63 padding
 * step_counter[1] (device int64: steps taken so far).  Every launch increments the counter and derives the last three floats
 * from the doubles ON the device with the code the eager entry point runs on the host; a changed hyper-parameter is carried
 * in by rewriting bytes 0 .. 47 on the replaying stream between two replays. */
int msn_adam_step_dev(const void* table, int n_tensors, int64_t max_numel, void* hyper, int decoupled,
                      long long* step_counter, msn_stream_t stream);
/* Fused multi-tensor SGD step: torch.optim's _single_tensor_sgd (not maximize).  table: DEVICE array of n_tensors
 * (1 .. 65535) records of four 64-bit words {p*, g*, buf*, numel}, buf = NULL without momentum; 20 B of HBM traffic /
 * parameter with momentum, 12 B without.  Per element:
 *   if (weight_decay != 0) grad = grad.add(param, alpha=weight_decay)              g = fma(wd, p, g)
 *   if (momentum != 0)  buf = clone(grad) the first time (first != 0), else
 *                       buf.mul_(momentum).add_(grad, alpha=1 - dampening)         buf = fma(momentum, buf, (1 - dampening) * g)
 *                       grad = nesterov ? grad.add(buf, alpha=momentum) : buf      g = nesterov ? fma(momentum, buf, g) : buf
 *   param.add_(grad, alpha=-lr)                                                    p = fma(-lr, g, p)
 * nesterov needs momentum > 0 and dampening == 0. */
int msn_sgd_step(const void* table, int n_tensors, int64_t max_numel, double lr, double momentum, double dampening,
                 double weight_decay, int nesterov, int first, msn_stream_t stream);
/* The recorded form.  hyper: DEVICE block of 64 bytes, 8-byte aligned: bytes 0 .. 31 double lr, momentum, dampening,
 * weight_decay; bytes 32 .. 47 float lr, momentum, 1 - dampening, weight_decay (rounded once by the host); bytes 48 .. 63
 * padding.  The launch only reads the block (SGD has no step count) and never takes the `first` branch: the momentum buffers
 * exist before the capture. */
int msn_sgd_step_dev(const void* table, int n_tensors, int64_t max_numel, void* hyper, int nesterov, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Layer-wise adaptive optimizers, LAMB and LARS (csrc/optim_layerwise.hip): per tensor a trust ratio from the 2-norms of the
 * whole tensor, the parameter's taken BEFORE the update.  One call = three multi-tensor launches over the table (fp32, n_tensors
 * 1 .. 65535, max_numel >= every numel): moments + per-block fp64 partial sums, one block per tensor that adds them in a fixed
 * order and writes the ratio, the update.
 * The multi-tensor launch rule (csrc/multi_tensor.h), shared by these steps, gradient clipping, gradient accumulation and weight
 * averaging below: grid y = tensor, grid x = blocks per tensor = ceil(max_numel / 4096), at most min(1024, max(32, 8192 /
 * n_tensors)) and at least 1; a block covers 4096 elements per pass and a larger tensor is covered in several passes.
 *   ws:    DEVICE scratch, 8-byte aligned, of msn_layerwise_workspace_bytes(n_tensors, max_numel) bytes or more.  The size
 *          never shrinks with more tensors or larger ones, so scratch sized for a param group serves any subset of it.
 *   ratio: n_tensors DEVICE floats: the trust ratios in table order, written by the second launch, read by the third and left
 *          for the caller.  They never visit the host: the calls can be recorded in a HIP graph.
 * Every scalar arrives in double and is rounded to float once; the ratio itself is formed in double from the exact scalars.
 *
 * msn_lamb_step: You et al. 2020 as timm's Lamb has it, without its gradient-norm pre-clipping.  table: records of five 64-bit
 * words {p*, g*, m*, v*, numel}; step is the 1-based update count; 40 B of HBM traffic / parameter.  With c1 = 1 - beta1^t and
 * c2 = 1 - beta2^t (both 1 when bias_correction == 0), 1 / c1 and sqrt(c2) formed in double:
 *   m = fma(1 - beta1, g - m, m)      [the fused lerp of msn_adam_step]        v = fma(beta2, v, ((1 - beta2) * g) * g)
 *   u = (m * (1 / c1)) / (sqrtf(v) / sqrt(c2) + eps);   if (weight_decay != 0) u = fma(weight_decay, p, u)
 *   ratio = ||p|| / ||u||  if (weight_decay != 0 or always_adapt) and ||p|| > 0 and ||u|| > 0, else 1;  trust_clip: min(ratio, 1)
 *   p = fma(-(lr * ratio), u, p)
 * u is formed twice, by one device function: for its norm in the first launch and again in the third, which reads the updated
 * m and v.  The gradient is never written.  A NaN norm fails the comparisons (ratio 1); the NaN reaches p through u. */
size_t msn_layerwise_workspace_bytes(int n_tensors, int64_t max_numel);
int msn_lamb_step(const void* table, int n_tensors, int64_t max_numel, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int bias_correction, int always_adapt, int trust_clip, int64_t step, void* ws,
                  size_t ws_bytes, float* ratio, msn_stream_t stream);
/* The same step for a training step recorded in a HIP graph.  hyper: DEVICE block of 64 bytes, 8-byte aligned:
 *   bytes  0 .. 31  double lr, beta1, beta2, weight_decay (exact)
 *   bytes 32 .. 55  float beta2, eps, 1 - beta1, 1 - beta2, lr, weight_decay (each rounded once from double by the host)
 *   bytes 56 .. 63  float 1 / c1, sqrt(c2) (written by every call)
 * step_counter[1] (device int64: steps taken so far).  Every call increments the counter from a one-thread launch and derives
 * the last two floats from the exact betas ON the device with the code msn_lamb_step runs on the host; a changed
 * hyper-parameter is carried in by rewriting bytes 0 .. 55 on the replaying stream between two replays. */
int msn_lamb_step_dev(const void* table, int n_tensors, int64_t max_numel, void* hyper, int bias_correction, int always_adapt,
                      int trust_clip, long long* step_counter, void* ws, size_t ws_bytes, float* ratio, msn_stream_t stream);
/* msn_lars_step: lightning-bolts' LARS, torch's SGD with a layer-wise rate on the decayed gradient.  table: records of four
 * 64-bit words {p*, g*, buf*, numel}, buf = NULL without momentum; 28 B of HBM traffic / parameter with momentum.
 *   ratio = trust_coefficient ||p|| / (||g|| + weight_decay ||p|| + eps)  if weight_decay != 0 and ||p|| > 0 and ||g|| > 0, else 1
 *   d = ratio * fma(weight_decay, p, g)                      [weight_decay == 0: d = g, and the step is msn_sgd_step's bit for bit]
 *   if (momentum != 0)  buf = d the first time (first != 0), else buf = fma(momentum, buf, (1 - dampening) * d)
 *                       d = nesterov ? fma(momentum, buf, d) : buf
 *   p = fma(-lr, d, p)
 * nesterov needs momentum > 0 and dampening == 0; trust_coefficient > 0. */
int msn_lars_step(const void* table, int n_tensors, int64_t max_numel, double lr, double momentum, double dampening,
                  double weight_decay, int nesterov, double trust_coefficient, double eps, int first, void* ws, size_t ws_bytes,
                  float* ratio, msn_stream_t stream);
/* The recorded form.  hyper: DEVICE block of 64 bytes, 8-byte aligned: bytes 0 .. 31 double lr, momentum, dampening,
 * weight_decay; bytes 32 .. 47 float lr, momentum, 1 - dampening, weight_decay (rounded once by the host); bytes 48 .. 63 double
 * trust_coefficient, eps.  The launches only read the block (LARS has no step count) and never take the `first` branch: the
 * momentum buffers exist before the capture. */
int msn_lars_step_dev(const void* table, int n_tensors, int64_t max_numel, void* hyper, int nesterov, void* ws, size_t ws_bytes,
                      float* ratio, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gradient clipping: torch.nn.utils.clip_grad_norm_ / clip_grad_value_ as pl.Trainer(gradient_clip_val=...,
 * gradient_clip_algorithm="norm" | "value") calls them after the gradient all-reduce and before optimizer.step().
 * table: DEVICE array of n_tensors (1 .. 65535) records of two 64-bit words {g*, numel} (fp32 gradients, in place);
 * max_numel >= every numel of the table.  One launch per pass for the whole model, by the multi-tensor launch rule above.
 *   msn_grad_norm: total_norm[0] = ||g||_p over all tensors (norm_type 1, 2 or INFINITY; NaN propagates) and
 *     coef[0] = min(max_norm / (total_norm + 1e-6), 1) (a NaN stays NaN), both DEVICE floats.  Per-block partials in fp64
 *     go to `ws` (msn_grad_norm_workspace_bytes: one double per block of the rule) and one block sums them in a fixed
 *     order: bitwise reproducible.
 *   msn_grad_scale: g *= coef[0] (the device-resident coefficient of msn_grad_norm).
 *   msn_grad_clamp: g = clamp(g, -clip_value, clip_value), NaN kept. */
size_t msn_grad_norm_workspace_bytes(int n_tensors, int64_t max_numel);
int msn_grad_norm(const void* table, int n_tensors, int64_t max_numel, float norm_type, float max_norm, float* total_norm,
                  float* coef, void* ws, size_t ws_bytes, msn_stream_t stream);
int msn_grad_scale(const void* table, int n_tensors, int64_t max_numel, const float* coef, msn_stream_t stream);
int msn_grad_clamp(const void* table, int n_tensors, int64_t max_numel, float clip_value, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gradient accumulation over micro-batches, pl.Trainer(accumulate_grad_batches=k): one launch per micro-batch for the whole
 * model in place of autograd's one add per parameter.
 * table: DEVICE array of n_tensors (1 .. 65535) records of four 64-bit words {dst*, acc*, g*, numel} (fp32);
 * max_numel >= every numel of the table (the multi-tensor launch rule).  Per element dst = g (store: the first micro-batch
 * of a window) or dst = acc + g
 * (add: one fp32 add, bitwise defined; NaN / inf as the add has them).  dst may be acc, g, or a third buffer.  A record whose
 * acc is NULL is stored in either mode; a store with dst == g moves nothing.
 * add: 0 = store, 1 = add.  add_dev: NULL, or a DEVICE int that overrides `add` (non-zero = add) -- a step recorded once in
 * a HIP graph is replayed at every position of a window, and the word is rewritten on the replaying stream between replays. */
int msn_grad_accumulate(const void* table, int n_tensors, int64_t max_numel, int add, const int* add_dev,
                        msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Weight averaging over training (Lightning's WeightAveraging / StochasticWeightAveraging, torch's AveragedModel): one launch
 * per optimizer step for every averaged tensor.
 * table: DEVICE array of n_tensors (1 .. 65535) records of three 64-bit words {avg*, p*, numel} (fp32);
 * max_numel >= every numel of the table (the multi-tensor launch rule).  state: two DEVICE 64-bit words {n_averaged, active}.
 *   active == 0: the launch changes nothing, neither the averages nor n_averaged;
 *   n_averaged == 0: avg = p, a copy of the bits;
 *   otherwise d = p - avg, avg = fmaf(w, d, avg), one rounding each, with
 *     MSN_AVG_EMA  w = weight = (float)(1.0 - decay), rounded once by the caller; 0 <= weight <= 1;
 *     MSN_AVG_SWA  w = (float)(1.0 / (double)(n_averaged + 1)), formed on the device (weight is ignored);
 *   then n_averaged += 1 (when active), by a one-thread kernel behind the main one on `stream`.
 *   MSN_AVG_SWAP  avg and p exchange their bits (twice is the identity); state may be NULL and is left alone.
 * `active` is meant to be rewritten on the replaying stream between the replays of a step recorded in a HIP graph. */
#define MSN_AVG_EMA 0
#define MSN_AVG_SWA 1
#define MSN_AVG_SWAP 2
int msn_weight_average(const void* table, int n_tensors, int64_t max_numel, int mode, float weight, long long* state,
                       msn_stream_t stream);

/* Channels-last convolution plumbing for the build-defined ResNet-18 / 1-D CNN encoders (not in the
 * reference): cols[(b,oh,ow)][(c,u,v)] = x[b, oh*sh+u-ph, ow*sw+v-pw, c] (0 outside), column order equal to
 * the flattening of a (C_out, C_in, kh, kw) weight, so conv = msn_sgemm(cols, W) ; col2im is its adjoint
 * (deterministic gather); a 1-D conv is the H = 1 case.  Max pooling keeps the arg-max pixel (int32). */
int msn_im2col(const float* x, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
               float* cols, msn_stream_t stream);
int msn_col2im(const float* dcols, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
               float* dx, msn_stream_t stream);
/* The same with TAP-MAJOR columns cols[(b,oh,ow)][(u,v,c)] (channels fastest: both kernels move 16-byte channel groups;
 * C % 4 == 0, 16-byte aligned tensors) and the weight re-laid to match: msn_conv_weight_relayout(to_tap = 1) copies
 * torch's (C_out, C_in, kh*kw) weight to (C_out, kh*kw, C_pad) with zeros in the channels C_in .. C_pad-1; to_tap = 0
 * is the inverse (for the weight gradient; the padding channels are dropped); to_tap = 2 gives (kh*kw, C_out, C_in)
 * (C_pad == C_in), the weight operand of msn_conv2d_dgrad.  msn_pad_channels widens a channels-last
 * tensor (rows x C -> rows x Cp, zeros added): a 3-channel image stem runs as a 4-channel convolution. */
int msn_im2col_tap(const float* x, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                   float* cols, msn_stream_t stream);
int msn_col2im_tap(const float* dcols, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                   float* dx, msn_stream_t stream);
int msn_conv_weight_relayout(const float* src, int64_t co, int ci, int ci_pad, int taps, int to_tap, float* dst,
                             msn_stream_t stream);
int msn_pad_channels(const float* x, int64_t rows, int C, int Cp, float* out, msn_stream_t stream);

/* Implicit-GEMM convolution on channels-last fp32 tensors (the build-defined ResNet-18 / 1-D CNN encoders; no
 * reference counterpart): y[(b,oh,ow)][co] = sum_{u,v,c} x[b, oh*sh+u-ph, ow*sw+v-pw, c] * w_tap[co][(u,v,c)] without a
 * column matrix in memory -- the GEMM kernel's LDS-DMA lanes compute their own source addresses and padding taps read
 * a page of zeros.  msn_conv2d_implicit_ok says whether a shape is taken (C and C_out multiples of 32 and > 32,
 * images up to 512 x 512, B*OH*OW a multiple of 32); other shapes go through msn_im2col_tap + msn_sgemm.
 *   fwd:   w_tap = msn_conv_weight_relayout(to_tap = 1) of the (C_out, C, kh, kw) weight; epilogue NONE or RELU.
 *   dgrad: stride 1 only; dx[(b,h,w)][c] from dy[(b,oh,ow)][co] and w_tco = relayout(to_tap = 2): [(u,v,co)][c].
 *   wgrad: dw_tap[co][(u,v,c)] (relayout(to_tap = 0) gives torch's layout back) and, when dbias != NULL, dbias[co] =
 *          column sums of dy from the same launch; split over the pixels, slabs in `ws`.
 * `ws` of msn_conv2d_workspace_bytes(...) bytes serves all three. */
int msn_conv2d_implicit_ok(int B, int H, int W, int C, int Cout, int kh, int kw, int sh, int sw, int ph, int pw);
size_t msn_conv2d_workspace_bytes(int B, int H, int W, int C, int Cout, int kh, int kw, int sh, int sw, int ph, int pw);
int msn_conv2d_fwd(const float* x, int B, int H, int W, int C, const float* w_tap, int Cout, int kh, int kw, int sh,
                   int sw, int ph, int pw, const float* bias, int epilogue, float* y, void* ws, size_t ws_bytes,
                   msn_stream_t stream);
int msn_conv2d_dgrad(const float* dy, int B, int H, int W, int C, const float* w_tco, int Cout, int kh, int kw, int ph,
                     int pw, float* dx, void* ws, size_t ws_bytes, msn_stream_t stream);
int msn_conv2d_wgrad(const float* dy, const float* x, int B, int H, int W, int C, int Cout, int kh, int kw, int sh,
                     int sw, int ph, int pw, float* dw_tap, float* dbias, void* ws, size_t ws_bytes,
                     msn_stream_t stream);
int msn_maxpool2d_fwd(const float* x, int B, int H, int W, int C, int k, int s, int p, float* y, int* argmax,
                      msn_stream_t stream);
int msn_maxpool2d_bwd(const float* dy, const int* argmax, int B, int H, int W, int C, int k, int s, int p,
                      float* dx, msn_stream_t stream);

/* nn.Dropout in train mode (src/transformer_utils.py:108,113,116,140; src/models_multimodal.py:71,78,87,850):
 * y = keep(seed, i) ? x / (1 - p) : 0 (+ residual), keep from a counter-based hash of (seed, element index), so the
 * same call applied to the gradient reproduces the mask and nothing is stored.  In place allowed. */
int msn_dropout(const float* x, int64_t n, float p, uint64_t seed, const float* residual, float* y,
                msn_stream_t stream);
/* For a training step recorded in a HIP graph: the seed is seed_base[0] (DEVICE memory) + seed_offset, and
 * msn_seed_advance (one launch per recorded step) moves the base, so every replay draws new masks while a forward
 * call and its backward twin (same offset) still agree. */
int msn_dropout_dev(const float* x, int64_t n, float p, const uint64_t* seed_base, uint64_t seed_offset,
                    const float* residual, float* y, msn_stream_t stream);
int msn_seed_advance(uint64_t* seed_base, msn_stream_t stream);

/* On-device form of NoisyDataLoader.__iter__ (src/dataloader.py:88-287), the step right before the path:
 *   images: out = rot90^{rot[b]}( img + (2 u - 1) * noise_level * std(img) )   (B, C, S, S), std = torch.std of the
 *           whole batch; u = uniform [0,1) field, rot = quarter turns per sample (both supplied by the caller's RNG);
 *   series: out = x + g * err * noise_level   (g = standard-normal field). */
size_t msn_augment_workspace_bytes(void);
int msn_augment_images(const float* img, const float* u, const int* rot, int64_t B, int C, int S,
                       float noise_level, float* out, void* ws, size_t ws_bytes, msn_stream_t stream);
int msn_augment_series(const float* x, const float* g, const float* err, int64_t n, float noise_level,
                       float* out, msn_stream_t stream);

/* Masked MSE of the masked-light-curve pretraining objective (src/models_pretraining.py:201-231):
 * stats[0] = mean over {i : select[i]} of (pred[i] - target[i])^2, stats[1] = number of selected elements;
 * bwd: dpred = grad_out * 2 (pred - target) / count on the selected elements, 0 elsewhere. */
int msn_masked_mse_fwd(const float* pred, const float* target, const uint8_t* select, int64_t n, float* stats,
                       msn_stream_t stream);
int msn_masked_mse_bwd(const float* pred, const float* target, const uint8_t* select, int64_t n,
                       const float* stats, const float* grad_out, float* dpred, msn_stream_t stream);

/* The masks of that objective, drawn on the device (csrc/pretrain_masks.hip): one launch, one workgroup per sample.
 *   pad (B, T) bytes: the padding mask (non-zero = observed); x (B, T) fp32 or NULL
 *   mask_in = the padding mask without the hidden points, mask_pred = the hidden points (bytes 0 / 1);
 *   x_masked = mask_in ? x : 0 (a select: a NaN at a hidden point leaves as 0), written only when x is given;
 *   starts (B, nbands) or NULL: the first position of every band's hidden run (contiguous mode only).
 * With mix(seed, c) = the 64-bit mixer of msn_dropout applied to c * 0x9E3779B97F4A7C15 + seed:
 *   MSN_MASK_CONTIGUOUS  get_continous_random_mask's rules (src/models_pretraining.py:58-98): band = T / nbands; in band k of
 *     sample i with n observed points, h = floor((double)n * f_mask) points from start = band k + mulhi64(mix(seed, i nbands + k),
 *     n - h + 1) on are hidden; positions at or behind band * nbands keep the padding mask in BOTH outputs.
 *   MSN_MASK_RANDOM  get_random_mask's meaning (:17-55): the h = floor(n_observed * f_mask) observed positions j of sample i that
 *     come first in the order by (mix(seed, i T + j), j) are hidden; nbands is not used (but checked).
 * T <= 4096, 1 <= nbands <= T, 0 <= f_mask <= 1, else MSN_ERR_SHAPE before any launch.  The _dev form takes the seed as
 * seed_base[0] (DEVICE memory) + seed_offset, as msn_dropout_dev does; for one seed value the two forms agree bit for bit. */
#define MSN_MASK_CONTIGUOUS 0
#define MSN_MASK_RANDOM 1
int msn_pretrain_masks(const uint8_t* pad, const float* x, int64_t B, int T, int nbands, double f_mask, int mode, uint64_t seed,
                       uint8_t* mask_in, uint8_t* mask_pred, float* x_masked, int32_t* starts, msn_stream_t stream);
int msn_pretrain_masks_dev(const uint8_t* pad, const float* x, int64_t B, int T, int nbands, double f_mask, int mode,
                           const uint64_t* seed_base, uint64_t seed_offset, uint8_t* mask_in, uint8_t* mask_pred,
                           float* x_masked, int32_t* starts, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Supervised heads on the towers (models_finetune.py: ClipMLP): classification / regression loss and validation metrics.
 * Cross-entropy with the semantics of torch.nn.functional.cross_entropy(logits, target, weight=w, reduction="mean"):
 * logits (N, C) fp32 with row stride ld, target int64 (N), weight (C) fp32 or NULL (= ones); 2 <= C <= 1024, N >= 1.
 * A target outside [0, C) -- torch's ignore_index -100 among them -- takes no part (numerator, denominator, gradient) and
 * is never used as an index.
 *   fwd: out[3] (DEVICE) = {loss, denom, numerator}: numerator = sum_i w[y_i] (lse_i - x[i, y_i]), denom = sum_i w[y_i],
 *        loss = numerator / (denom_in ? denom_in[0] : denom) -- denom_in: a DEVICE scalar of the caller's for a mean over
 *        more rows than this call sees, when it is known before the call (models_finetune.py passes NULL: under data
 *        parallel the ranks' denominator exists only after this forward, so it divides out[2] by the all-reduced out[1]
 *        itself and hands that sum to bwd as `denom`); all rows ignored gives nan.  Also lse[i] (N) and
 *        pred[i] = argmax_c x[i, c] (int32, first maximal index).  Row terms in fp32 (max subtracted, expf / log1pf), sums over
 *        rows in fp64: ONE launch up to N = 4096 (C <= 16) / N = 64 (wider rows), else per-block partials in `ws`
 *        (msn_cross_entropy_workspace_bytes) + one finishing block that adds them in a fixed order.  Bitwise reproducible.
 *   bwd: dlogits[i, c] = grad_out[0] * w[y_i] * (softmax(x_i)[c] - [c == y_i]) / denom[0] (DEVICE scalars; rows of an
 *        ignored target are zeroed), one launch.  The softmax is recomputed from the logits, not from the fp32 lse
 *        (which rounds to 4e-6 for logits of magnitude 60). */
size_t msn_cross_entropy_workspace_bytes(int64_t N, int C);
int msn_cross_entropy_fwd(const float* logits, int64_t ld, const int64_t* target, const float* weight, int64_t N, int C,
                          const float* denom_in, float* lse, int* pred, float* out, void* ws, size_t ws_bytes,
                          msn_stream_t stream);
int msn_cross_entropy_bwd(const float* logits, int64_t ld, const int64_t* target, const float* weight, int64_t N, int C,
                          const float* denom, const float* grad_out, float* dlogits, int64_t lddx, msn_stream_t stream);
/* Focal loss with label smoothing (csrc/focal_loss.hip; models_finetune.py: focal_loss, cross_entropy(label_smoothing > 0)).
 * Arguments as msn_cross_entropy_*: logits (N, C) fp32 with row stride ld, target int64 (N), weight (C) fp32 or NULL (= ones).
 * With p = softmax(x_i), u_c = 1 - p_c and q_c = (1 - label_smoothing) [c == y_i] + label_smoothing / C,
 *   numerator = sum_i sum_c q_c w_c u_c^gamma (-log p_c),   denom = sum_i w[y_i]      (rows with 0 <= y_i < C only)
 * gamma = 0 is torch's cross_entropy(weight=w, label_smoothing=, reduction="mean"); label_smoothing = 0 is the multiclass
 * focal loss w_y (1 - p_y)^gamma (-log p_y).  A target outside [0, C) takes no part and is never used as an index.
 *   fwd: out[3] (DEVICE, fp32) = {numerator / (denom_in ? denom_in[0] : denom), denom, numerator}; all rows ignored gives nan.
 *        pred[i] = argmax_c x[i, c] (int32; a NaN beats every number, the first index wins a tie).  ONE launch up to
 *        N = 256 (C <= 16) / N = 4 (wider rows) -- one row per lane / wave of a 256-thread workgroup; the fp64 rows make a
 *        larger single workgroup slower than several -- else per-block fp64 partials in `ws`
 *        (msn_focal_loss_workspace_bytes) + one finishing block that adds them in a fixed order.
 *   bwd: dlogits (N, C) fp32 with row stride lddx = grad_out[0] * d numerator / d logits / denom[0] (DEVICE scalars); the
 *        rows are recomputed from the logits, rows of an ignored target are zeroed; one launch.
 * Row arithmetic in fp64 from the fp32 logits, u and log p formed without cancellation; out and dlogits are rounded to fp32
 * once.  No atomics: bitwise reproducible, for every row stride.
 * MSN_ERR_SHAPE before any launch (the workspace query returns 0): C outside 2..1024, N outside 1..2^31 - 1, gamma not finite
 * or < 0, label_smoothing outside [0, 1], a row stride below C, a null or misaligned pointer, a workspace that is too small. */
size_t msn_focal_loss_workspace_bytes(int64_t N, int C);
int msn_focal_loss_fwd(const float* logits, int64_t ld, const int64_t* target, const float* weight, int64_t N, int C,
                       double gamma, double label_smoothing, const float* denom_in, int* pred, float* out, void* ws,
                       size_t ws_bytes, msn_stream_t stream);
int msn_focal_loss_bwd(const float* logits, int64_t ld, const int64_t* target, const float* weight, int64_t N, int C,
                       double gamma, double label_smoothing, const float* denom, const float* grad_out, float* dlogits,
                       int64_t lddx, msn_stream_t stream);
/* cm[target[i], pred[i]] += 1 for every row with both in [0, C): cm a caller-owned (C, C) int32 DEVICE matrix that
 * accumulates over calls (MulticlassFBetaScore / accuracy are formed from it on the host).  Integer adds only; up to
 * C = 64 every workgroup counts in its own LDS copy and adds each non-zero cell once. */
int msn_confusion_matrix(const int64_t* target, const int* pred, int64_t N, int C, int* cm, msn_stream_t stream);
/* acc[6] (DEVICE, fp64, caller-owned, accumulates over calls) += {n, sum|d|, sum d^2, sum y, sum y^2, n_out} with
 * d = pred - y formed in fp64 and n_out = rows with |d| / (1 + y) > 0.15 (the outlier fraction of photometric redshifts).
 * Per-block fp64 partials in `ws` (msn_regression_stats_workspace_bytes; none up to N = 4096) + one finishing block. */
size_t msn_regression_stats_workspace_bytes(int64_t N);
int msn_regression_stats(const float* pred, const float* target, int64_t N, double* acc, void* ws, size_t ws_bytes,
                         msn_stream_t stream);
/* Robust, Gaussian-NLL and quantile losses for the redshift head (csrc/regression_loss.hip; models_finetune.py:
 * regression_loss).  pred (N, K) fp32 with row stride ld >= K, target (N) fp32.  A row is VALID when its target is finite: a
 * NaN or infinite target (an object without a spectroscopic redshift) adds nothing to numerator or denominator and its
 * gradient row is exactly zero.  With d = pred - y, per valid row:
 *   MSE (K = 1) d^2 | L1 (K = 1) |d|, gradient 0 at d = 0 | HUBER (K = 1, delta > 0) d^2 / 2 up to |d| = delta, else
 *   delta (|d| - delta / 2) | LOG_COSH (K = 1) log cosh d = log1p(2 sinh^2(d / 2)) up to |d| = 1, |d| + log1p(e^{-2|d|}) - ln 2
 *   beyond | GAUSSIAN_NLL (K = 2: mu, s = log variance) (s + (mu - y)^2 e^-s) / 2 | PINBALL (1 <= K <= 16, levels taus[K],
 *   DEVICE fp64, strictly increasing inside (0, 1) -- checked by the caller, not here) (1 / K) sum_q max(tau_q e_q,
 *   (tau_q - 1) e_q) with e_q = y - pred_q, gradient 0 at e_q = 0.  delta is read by HUBER and taus by PINBALL only.
 *   fwd: out[3] (DEVICE, fp32) = {numerator / (denom_in ? denom_in[0] : denom), denom, numerator}, denom = the number of valid
 *        rows (an exact integer carried in fp64); no valid row gives nan.  ONE launch up to N = 256 (one row per lane of a
 *        256-thread workgroup), else per-block fp64 partials in `ws` (msn_regression_loss_workspace_bytes) + one finishing
 *        block that adds them in a fixed order.
 *   bwd: dpred (N, K) fp32 with row stride lddx = grad_out[0] * d numerator / d pred / denom[0] (DEVICE scalars); the rows
 *        are recomputed, rows of an ignored target are zeroed; one launch.
 * Row arithmetic in fp64 from the fp32 inputs; out and dpred are rounded to fp32 once.  Non-finite predictions propagate;
 * e^-s overflows for s < -709 and propagates too.  No atomics, 4-byte loads of pred and target: bitwise reproducible, for
 * every row stride and every 4-byte alignment.
 * MSN_ERR_SHAPE before any launch (the workspace query returns 0): an unknown kind, K not matching the kind or outside 1..16,
 * N outside 1..2^31 - 1, delta not finite or <= 0 for HUBER, null taus for PINBALL, a row stride below K, a null or
 * misaligned pointer, a workspace that is too small. */
#define MSN_REGLOSS_MSE 0
#define MSN_REGLOSS_L1 1
#define MSN_REGLOSS_HUBER 2
#define MSN_REGLOSS_LOG_COSH 3
#define MSN_REGLOSS_GAUSSIAN_NLL 4
#define MSN_REGLOSS_PINBALL 5
size_t msn_regression_loss_workspace_bytes(int64_t N, int K);
int msn_regression_loss_fwd(const float* pred, int64_t ld, const float* target, int64_t N, int K, int kind, double delta,
                            const double* taus, const float* denom_in, float* out, void* ws, size_t ws_bytes,
                            msn_stream_t stream);
int msn_regression_loss_bwd(const float* pred, int64_t ld, const float* target, int64_t N, int K, int kind, double delta,
                            const double* taus, const float* denom, const float* grad_out, float* dpred, int64_t lddx,
                            msn_stream_t stream);
/* Validation statistics of those heads over the valid rows, added to two caller-owned DEVICE buffers that persist over calls:
 * acc[8] fp64 and cnt[19] int64.  acc[0..5] are msn_regression_stats' six sums {n, sum|d|, sum d^2, sum y, sum y^2, n_out} of
 * the point prediction; cnt[0] = n.
 *   POINT (K = 1):     the point prediction is pred itself; acc[6], acc[7] stay.
 *   GAUSSIAN (K = 2):  the point prediction is mu; acc[6] += sum sigma, acc[7] += sum z^2 (sigma = e^{s / 2}, z = d / sigma);
 *                      cnt[k] += rows with |d| <= k sigma, k = 1, 2, 3 (fp64 compare).
 *   QUANTILE (K <= 16): the point prediction is column `mid`; acc[6] += sum (pred_{K-1} - pred_0), acc[7] += sum of the row
 *                      pinball terms (taus as above); cnt[1] += rows with pred_0 <= y <= pred_{K-1}, cnt[2] += rows with some
 *                      pred_q > pred_{q+1}, cnt[3 + q] += rows with y <= pred_q (IEEE fp32 compares: a NaN is below nothing).
 * One launch up to N = 256, else per-block fp64 partials in `ws` + one finishing block (fixed order); the counts are integer
 * adds, which commute: workgroup order, the cut of an epoch into calls and a SUM all-reduce change no bit of them. */
#define MSN_REGSTATS_POINT 0
#define MSN_REGSTATS_GAUSSIAN 1
#define MSN_REGSTATS_QUANTILE 2
size_t msn_regression_interval_stats_workspace_bytes(int64_t N);
int msn_regression_interval_stats(const float* pred, int64_t ld, const float* target, int64_t N, int K, int mode, int mid,
                                  const double* taus, int64_t* cnt, double* acc, void* ws, size_t ws_bytes,
                                  msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Linear probes on frozen embeddings (probes.py; csrc/probes.hip): the two fp64 reductions a probe fit needs.  An fp32
 * value times an fp32 value is exact in fp64, so only the additions round; their order is a function of the shape alone
 * (per-slab / per-block fp64 partials in `ws`, added in a fixed order by a finishing launch: sixteen -- four up to eight
 * partials -- interleaved groups, each in slab / block order, then the groups in group order), so the results repeat
 * bit for bit from run to run and from device to device.  Two launches per call, no fills, no float atomics.
 *
 * Gram: G (M, M) fp64 row-major, M = D + 1 + K, receives Z^T Z for Z = [X | 1 | Y] assembled on the fly (Z is never
 * written): X (N, D) fp32 with row stride ldx >= D, Y (N, K) fp32 with row stride ldy >= K, or NULL with K = 0; both
 * 4-byte aligned (every load is a 4-byte load: the bits do not depend on stride or alignment).  accumulate = 0 stores
 * the result, accumulate = 1 adds it to what G holds.  G[i][j] and G[j][i] are written from the same sum.  One matrix so
 * carries X^T X, the column sums, n, X^T Y, 1^T Y and Y^T Y.  1 <= D <= 1024, 0 <= K <= 16, N >= 1, else MSN_ERR_SHAPE.
 * msn_probe_gram_slab_rows: the rows of one slab for that shape (the partial sums change hands at its multiples). */
int64_t msn_probe_gram_slab_rows(int64_t N, int D, int K);
size_t msn_probe_gram_workspace_bytes(int64_t N, int D, int K);
int msn_probe_gram(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, int K, double* G,
                   int accumulate, void* ws, size_t ws_bytes, msn_stream_t stream);
/* Multinomial logistic regression, loss and gradient in one evaluation: y int64 (N), class_weight C doubles or NULL
 * (= ones), W (C, D + 1) fp64 row-major with the intercept in the last column, z_r = W [x_r | 1];
 *   out[0] = sum_r w[y_r] (lse(z_r) - z_r[y_r]),   out[1 + c (D + 1) + d] = sum_r w[y_r] (softmax(z_r) - e_{y_r})[c] [x_r | 1][d]
 * (1 + C (D + 1) doubles).  Everything in fp64: logits by fma, exp / log of the device math library on max-subtracted
 * logits.  A row whose target lies outside [0, C) contributes nothing.  No regularisation term: the host adds it.
 * 2 <= C, 1 <= D <= 1024, C (D + 1) <= 16400 (W stays in LDS as doubles), N >= 1, else MSN_ERR_SHAPE.
 * msn_logreg_block_rows: the rows one workgroup owns for that shape. */
int64_t msn_logreg_block_rows(int64_t N, int D, int C);
size_t msn_logreg_workspace_bytes(int64_t N, int D, int C);
int msn_logreg_loss_grad(const float* X, int64_t ldx, const int64_t* y, const double* class_weight, int64_t N, int D, int C,
                         const double* W, double* out, void* ws, size_t ws_bytes, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Exact k-nearest-neighbour search and kNN prediction on frozen embeddings (probes.py; csrc/knn.hip).
 *
 * Search: for fp32 queries Q (Nq, D), row stride ldq >= D, and a fp32 training set X (Nx, D), row stride ldx >= D, both
 * 4-byte aligned (every load is a 4-byte load), idx (Nq, k) int32 and dist2 (Nq, k) fp64, both dense, receive per query the
 * k training rows of smallest squared Euclidean distance, ascending.
 *   Membership is decided on |q|^2 + |x|^2 - 2 q.x in fp64 (dot products on the fp64 matrix cores; an fp32 value times an
 *   fp32 value is exact in fp64, so only the additions round, in an order that is a function of D alone), under the key
 *   (d2, index), lower index first: a strict total order, so the k winners do not depend on how the rows are cut into
 *   tiles and slabs.  Two rows whose true distances differ by less than the expansion's error (about
 *   (D + 4) 2^-52 (|q|^2 + |x|^2)) may change places at the k-th position; exact ties never do.
 *   dist2 is then recomputed for the k winners as sum_c (q_c - x_c)^2 by fma over c = 0 .. D - 1 in fp64: non-negative, 0 for
 *   identical rows, and its bits depend on the two rows and D only -- not on Nq, Nx, position, stride or alignment.  The k
 *   are sorted by (that value, index).  A NaN distance sorts last among the real rows.
 *   self_offset: -1 for none; otherwise the candidate j == i + self_offset is skipped for query i (leave-one-out when the
 *   queries are the training rows X[self_offset : self_offset + Nq]), and k <= Nx - 1 is required.
 *   Per-slab lists of k keys per query sit in `ws` (msn_knn_workspace_bytes = 12 Nq slabs k bytes, rounded up to 8); the
 *   Nq x Nx distances are never written to memory.  Two launches, no atomics, no fills: the same bits on every run.
 *   1 <= D <= 1024, 1 <= k <= 64, k <= Nx (Nx - 1 with self_offset >= 0), Nx < 2^31, Nq >= 1, else MSN_ERR_SHAPE before any launch.
 * msn_knn_slab_rows: the training rows one workgroup scans for that shape (the per-slab lists change hands at its multiples). */
int64_t msn_knn_slab_rows(int64_t Nq, int64_t Nx, int D, int k);
size_t msn_knn_workspace_bytes(int64_t Nq, int64_t Nx, int D, int k);
int msn_knn_search(const float* Q, int64_t ldq, int64_t Nq, const float* X, int64_t ldx, int64_t Nx, int D, int k,
                   int64_t self_offset, int* idx, double* dist2, void* ws, size_t ws_bytes, msn_stream_t stream);
/* Prediction from a search's (idx, dist2), one launch each.  weights = 0: every neighbour weighs 1; weights = 1: 1 / sqrt(dist2),
 * and where any of a query's k distances is 0 its zero-distance neighbours weigh 1 and the others 0 (scikit-learn's rule).
 * Sums are fp64 and run in neighbour order t = 0 .. k - 1.
 * Regression: Y (Nx, K) fp32, row stride ldy, 1 <= K <= 16; out (Nq, K) fp32, row stride ldo, = sum_t w_t y_t / sum_t w_t,
 * rounded once to fp32 (uniform weights: the fp64 mean of the k targets). */
int msn_knn_predict_regression(const int* idx, const double* dist2, int64_t Nq, int k, const float* Y, int64_t ldy, int K,
                               int weights, float* out, int64_t ldo, msn_stream_t stream);
/* Classification: y (Nx) int64 labels, 1 <= C <= 1024 classes; classes (Nq) int32 = the class of the largest vote (fp64 sums
 * of the weights), the lowest class on equal votes; proba_or_null (Nq, C) fp32 dense = vote / sum of the votes (0 where no
 * neighbour carries a label in range).  A label outside [0, C) is not an error here: it counts for no class. */
int msn_knn_predict_classes(const int* idx, const double* dist2, int64_t Nq, int k, const int64_t* y, int C, int weights,
                            int* classes, float* proba_or_null, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pair sums over embeddings (embedding_metrics.py; csrc/embedding_metrics.hip): what alignment and uniformity are made of.
 *
 * Potential: X (Nx, D) and Y (Ny, D) fp32, row strides ldx, ldy >= D, 4-byte aligned (every load is a 4-byte load: the bits do
 *   not depend on stride or alignment).  out (2 doubles) receives out[0] = sum_S exp(-t d2_ij) and out[1] = sum_S d2_ij with
 *   d2_ij = max(0, |x_i|^2 + |y_j|^2 - 2 x_i.y_j) in fp64, over the pair set S of `mode`:
 *     0  all Nx Ny pairs;   1  the same without i == j (Nx == Ny);   2  the unordered pairs i < j within X (Y == NULL, Ny == 0,
 *     Nx >= 2): only the tile pairs on or above the diagonal are computed.
 *   d2 is formed as msn_knn_search forms it: 64 x 64 tiles of dot products on the fp64 matrix instruction, norms by fma chains
 *   over the same staged columns, D never split and padded with zeros, so every d2 depends on the two rows and D alone.  exp is
 *   the device library's fp64 exp.  A row past Nx / Ny is never a pair.  The Nx x Ny matrix is never written.
 *   Sums: tile pairs are numbered row by row; workgroup b owns the pairs b per .. (b + 1) per - 1, per = ceil(pairs / 1024),
 *   blocks = ceil(pairs / per), pairs = ceil(Nx / 64) ceil(Ny / 64) (mode 2: T (T + 1) / 2, T = ceil(Nx / 64)).  A lane adds its
 *   16 pairs per tile in tile order, the workgroup's 256 lanes are reduced (xor tree, then the four waves in order) into one
 *   partial pair in `ws` (16 blocks bytes), and one finishing workgroup adds partial u, u + 256, ... in thread u and reduces alike.
 *     A(Nx, Ny, mode) = 16 per + 9 + ceil(blocks / 256) + 9
 *   is the largest number of additions any single term passes through on its way to out: every term is non-negative, so
 *   out[0] and out[1] carry a relative error of at most A 2^-53 from the summation (first order).
 *   Two launches, no atomics, no fills: the same bits on every run.  Non-finite inputs are not checked and propagate.
 *   MSN_ERR_SHAPE before any launch: D outside 1..1024, Nx < 1, Ny < 1 in modes 0 / 1, Nx != Ny in mode 1, Nx < 2 or Y != NULL
 *   or Ny != 0 in mode 2, Nx or Ny >= 2^31, t not finite or <= 0, an unknown mode, a workspace that is too small.
 * Alignment: d2_i = sum_c (x_ic - y_ic)^2 by fma in column order (the direct form of the kNN finish: non-negative, exactly 0 for
 *   identical rows); out[0] = sum_i d2_i, out[1] = sum_i sqrt(d2_i); d2_rows_or_null, where given, receives the N values.
 *   Thread u of workgroup b adds the rows (b + k blocks) 256 + u, k = 0, 1, ..., blocks = min(ceil(N / 256), 1024); then the same
 *   two reductions.  1 <= D <= 1024, 1 <= N < 2^31, else MSN_ERR_SHAPE before any launch. */
size_t msn_pair_potential_workspace_bytes(int64_t Nx, int64_t Ny, int D, int mode);
int msn_pair_potential(const float* X, int64_t ldx, int64_t Nx, const float* Y, int64_t ldy, int64_t Ny, int D, double t, int mode,
                       double* out, void* ws, size_t ws_bytes, msn_stream_t stream);
size_t msn_pair_alignment_workspace_bytes(int64_t N, int D);
int msn_pair_alignment(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, double* out,
                       double* d2_rows_or_null, void* ws, size_t ws_bytes, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Alignment + uniformity as a training loss (loss.py, embedding_metrics.py; csrc/uniformity_loss.hip).
 *
 * Row field: X (Nx, D) and Y (Ny, D) fp32, row strides ldx, ldy >= D, 4-byte aligned (every load is a 4-byte load), Y may alias
 *   X.  With w_ij = exp(-t d2_ij), d2_ij and exp exactly as msn_pair_potential forms them (the same bits), over the rows j of Y
 *   but j == i + self_offset (self_offset >= 0; -1 leaves nothing out):
 *     r (Nx) fp64        r_i  = sum_j w_ij
 *     F (Nx, D) fp64     F_ic = fma(r_i, x_ic, -M_ic),  M_ic = sum_j w_ij y_jc      (= sum_j w_ij (x_ic - y_jc), dense rows)
 *   M is a second product on the fp64 matrix instruction chained behind the scores: the 64 x 64 tile of w goes through LDS and
 *   becomes the A operand, the Y tile is staged again chunk by chunk, the 64 x D accumulator stays in registers.  The Nx x Ny
 *   matrix is never written; a row past Nx is never written, a row past Ny contributes nothing.
 *   Plan: workgroup (ti, s) owns row tile ti and the column tiles s per .. (s + 1) per - 1 with TI = ceil(Nx / 64),
 *   TJ = ceil(Ny / 64), per = ceil(TJ / min(TJ, ceil(512 / TI))), slabs = ceil(TJ / per): a function of (Nx, Ny), no device
 *   query.  Per-slab partials sit in `ws` (msn_pair_field_workspace_bytes = 8 slabs Nx (D + 1) bytes); the finishing launch adds
 *   them in slab order.
 *     A_f(Nx, Ny) = 64 per + slabs
 *   is the largest number of additions any single term passes through on its way to r_i or M_ic (4 per matrix instruction, 16
 *   instructions per column tile; r's own chain is shorter).  The terms of r_i are non-negative: r_i carries a relative error of
 *   A_f 2^-53 from the summation; M_ic one of A_f 2^-53 sum_j w_ij |y_jc|; F_ic one more rounding (the fma).
 *   Two launches, no atomics, no fills: the same bits on every run and for every stride or alignment.  Non-finite inputs are
 *   not checked and propagate.
 *   MSN_ERR_SHAPE before any launch: D outside 1..256, Nx or Ny < 1 or >= 2^31, t not finite or <= 0, self_offset < -1, a null
 *   pointer, a row stride below D, a workspace that is too small.
 * Loss, N >= 2 partner rows: L = (1 / N) sum_i |x_i - y_i|^alpha + lam / 2 (U_x + U_y), U = log(2 S / (N (N - 1))),
 *   S = sum_i r_i / 2 with r_x, r_y the fields of X and of Y against themselves with self_offset 0.
 *   Forward (two launches): d2_i by fma in column order and the three sums over the rows in the order of msn_pair_alignment
 *   (thread u of workgroup b adds the rows (b + k blocks) 256 + u; the xor tree, the four waves in order; one finishing workgroup
 *   likewise).  loss (1 float) is rounded once from fp64; comp (5 doubles) = (align, U_x, U_y, S_x, S_y); d2_rows (N doubles) is
 *   kept for the backward.  ws: msn_align_uniform_workspace_bytes(N) = 24 min(ceil(N / 256), 1024) bytes.
 *   Backward (one launch), from the saved F_x, F_y (N, D dense), d2_rows, comp and the device scalar g (1 float):
 *     dX_ic = fl32(g (k_i (x_ic - y_ic) - lam t Fx_ic / S_x)),  dY_ic = fl32(g (-k_i (x_ic - y_ic) - lam t Fy_ic / S_y)),
 *   k_i = 2 / N (alpha 2) or 1 / (N sqrt(d2_i)) (alpha 1; 0 where d2_i == 0), evaluated in fp64.  S == 0 (every w underflowed)
 *   is not checked: U is -inf and the gradient is not finite.  No host read: the step records into a graph.
 *   MSN_ERR_SHAPE before any launch: D outside 1..256, N < 2 or >= 2^31, alpha not 1 or 2, lam negative or not finite, t not
 *   finite or <= 0 (backward), a null pointer, a row stride below D, a workspace that is too small. */
size_t msn_pair_field_workspace_bytes(int64_t Nx, int64_t Ny, int D);
int msn_pair_field(const float* X, int64_t ldx, int64_t Nx, const float* Y, int64_t ldy, int64_t Ny, int D, double t,
                   int64_t self_offset, double* r, double* F, void* ws, size_t ws_bytes, msn_stream_t stream);
size_t msn_align_uniform_workspace_bytes(int64_t N);
int msn_align_uniform_fwd(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, const double* r_x,
                          const double* r_y, int alpha, double lam, float* loss, double* comp, double* d2_rows, void* ws,
                          size_t ws_bytes, msn_stream_t stream);
int msn_align_uniform_bwd(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, const double* F_x,
                          const double* F_y, const double* d2_rows, const double* comp, const float* g, int alpha, double t,
                          double lam, float* dX, int64_t lddx, float* dY, int64_t lddy, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * VICReg (Bardes, Ponce, LeCun 2022) as a training loss (loss.py; csrc/vicreg.hip): the centred column covariance, the loss
 * and the product of its gradient.  X, Y (N, D) fp32 with row strides >= D, 4-byte aligned, not assumed unit-norm;
 * 2 <= N < 2^31, 1 <= D <= 256.  Everything below is fp64 on the device, enqueue only, no atomics, no fills, no zeroed
 * scratch; every load of X and Y is a 4-byte load, so the bits depend on the values, N and D only (not on stride, alignment
 * or run).  Non-finite inputs are not checked and propagate.
 *
 * Column covariance: mean (D) and cov (D x D, symmetric bit for bit) of X,
 *   mean_c = (1 / N) sum_i x_ic      cov_cc' = (1 / (N - 1)) sum_i (x_ic - mean_c)(x_ic' - mean_c')
 *   Plan, a function of (N, D) alone (no device query):
 *     means: mrows = max(64, ceil(N / 64)) rows per slab, mslabs = ceil(N / mrows); a thread adds one column of its slab in row
 *     order, the slabs are added in slab order from slab 0 on, then one division by N;
 *     Gram: T = ceil(D / 64) column tiles, pairs = T (T + 1) / 2 tile pairs on or above the diagonal (nothing below it is
 *     computed), chunks = ceil(N / 32), per = max(4, ceil(chunks / ceil(512 / pairs))), slabs = ceil(chunks / per): workgroup
 *     (pair, slab) multiplies the 32 per rows of its slab on v_mfma_f64_16x16x4_f64, the rows staged as doubles with the mean
 *     subtracted on the way into LDS (one rounding per element; no X^T X - N mean mean^T cancellation); the finishing launch
 *     adds the slabs' partials in slab order, divides by N - 1 and writes (c, c') and (c', c) from the same numbers.
 *   Additions at most on a term's way
 *     to a mean:                A_mean(N)   = mrows + mslabs
 *     to a covariance entry:    A_cov(N, D) = 32 per + slabs     (4 per matrix instruction, 8 instructions per 32 rows, the slabs)
 *   ws: msn_column_cov_workspace_bytes = 8 (mslabs D + 4096 slabs pairs) bytes.  Three launches.
 *
 * Forward (three launches): inv = (1 / (N D)) sum_ic (x_ic - y_ic)^2 with d2_i by fma in column order and the sum over the rows
 *   in the order of msn_pair_alignment; over the two covariance matrices, s_c = sqrt(C_cc + eps),
 *     var = (1 / D) sum_c max(0, gamma - s_c)      cov = (1 / D) sum_{c != c'} C_cc'^2   (C^2 added by fma)
 *   one entry per thread and step over blocks = min(ceil(D^2 / 256), 64) workgroups, the xor tree, the four waves in order, one
 *   finishing workgroup likewise:
 *     to a sum over D x D:      A_dd(D)     = ceil(D^2 / (256 blocks)) + 9 + ceil(blocks / 256) + 9
 *   comp (5 doubles) = (inv, var_x, var_y, cov_x, cov_y); loss (1 float) = sim inv + std (var_x + var_y) + covc (cov_x + cov_y),
 *   rounded once from fp64; M_x, M_y (D x D doubles) are the coefficient matrices of the backward,
 *     M = (4 covc / (D (N - 1))) offdiag(C) - diag(std [s_c < gamma] / (D (N - 1) s_c))
 *   (the hinge is inactive at s_c == gamma).  ws: msn_vicreg_workspace_bytes = 8 (min(ceil(N / 256), 1024) + 4 blocks) bytes.
 * Backward (one launch): P = (X - mean) M on the same instruction, a 64 x 64 tile of P per workgroup, its fp64 accumulator in
 *   registers, the centred rows staged 32 inner columns at a time and M in chunks of 32 x 64 through LDS,
 *     to an entry of P:         A_p(D)      = 32 ceil(D / 32)
 *   dX = fl32(g (k (x - y) + P_x)), dY = fl32(g (-k (x - y) + P_y)), k = 2 sim / (N D), g a DEVICE float.  It reads X, Y, the
 *   means and M_x, M_y only.  Rows past N are never read and never written (dX, dY have row strides lddx, lddy >= D).
 * No host read anywhere: the step records into a graph.
 * MSN_ERR_SHAPE before any launch: D outside 1..256, N < 2 or >= 2^31, a coefficient negative or not finite, gamma negative
 * or not finite, eps not finite or <= 0, a null pointer, a misaligned pointer, a row stride below D, a workspace that is too
 * small. */
size_t msn_column_cov_workspace_bytes(int64_t N, int D);
int msn_column_cov(const float* X, int64_t ldx, int64_t N, int D, double* mean, double* cov, void* ws, size_t ws_bytes,
                   msn_stream_t stream);
size_t msn_vicreg_workspace_bytes(int64_t N, int D);
int msn_vicreg_fwd(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, const double* cov_x,
                   const double* cov_y, double sim_coeff, double std_coeff, double cov_coeff, double gamma, double eps, float* loss,
                   double* comp, double* M_x, double* M_y, void* ws, size_t ws_bytes, msn_stream_t stream);
int msn_vicreg_bwd(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, const double* mean_x,
                   const double* mean_y, const double* M_x, const double* M_y, const float* g, double sim_coeff, float* dX,
                   int64_t lddx, float* dY, int64_t lddy, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Barlow Twins (Zbontar et al. 2021) as a training loss (loss.py; csrc/barlow.hip): the centred cross covariance of two towers
 * with their biased variances, the loss and the product of its gradient.  X, Y (N, D) fp32 with row strides >= D, 4-byte
 * aligned, not assumed unit-norm; 2 <= N < 2^31, 1 <= D <= 256.  Everything below is fp64 on the device, enqueue only, no
 * atomics, no fills, no zeroed scratch; every load of X and Y is a 4-byte load, so the bits depend on the values, N and D only
 * (not on stride, alignment or run).  Non-finite inputs are not checked and propagate.
 *
 *   mean_x, mean_y column means, Xc = X - mean_x, Yc = Y - mean_y
 *   v_x[a] = (1 / N) sum_i Xc_ia^2    s_x[a] = sqrt(v_x[a] + eps)     (BatchNorm1d(affine=False): biased, eps inside the root)
 *   cov[a][b] = (1 / N) sum_i Xc_ia Yc_ib  (D x D, not symmetric)     c[a][b] = cov[a][b] / (s_x[a] s_y[b])
 *   on = sum_a (c_aa - 1)^2    off = sum_{a != b} c_ab^2    L = on + lambd off
 *   G_ab = 2 (c_aa - 1) if a == b else 2 lambd c_ab    A_ab = G_ab / (N s_x[a] s_y[b])    r_a = sum_b G_ab c_ab    q_b = sum_a G_ab c_ab
 *   dL/dX = Yc A^T + Xc diag(d_x), d_x[a] = -r_a / (N (v_x[a] + eps))    dL/dY = Xc A + Yc diag(d_y), d_y[b] = -q_b / (N (v_y[b] + eps))
 *   (BatchNorm's mean_i(dL/dxhat) term combines the column means of the standardised partner, which are zero: left out.)
 *
 * Cross covariance (three launches): mean_x, mean_y, var_x, var_y (D each) and cov (D x D).
 *   Plan, a function of (N, D) alone (no device query):
 *     means: mrows = max(64, ceil(N / 64)) rows per slab, mslabs = ceil(N / mrows); a thread adds one column of its slab in row
 *     order, the slabs are added in slab order from slab 0 on, then one division by N (as msn_column_cov);
 *     Gram: T = ceil(D / 64) column tiles, pairs = T^2 tile pairs (a, b), pair = a T + b (every pair is distinct), chunks =
 *     ceil(N / 32), per = max(4, ceil(chunks / ceil(512 / pairs))), slabs = ceil(chunks / per): workgroup (pair, slab) multiplies
 *     the 32 per rows of its slab on v_mfma_f64_16x16x4_f64, tile a of X against tile b of Y, staged as doubles with the mean
 *     subtracted on the way into LDS (one rounding per element; no X^T Y - N mean_x mean_y^T cancellation);
 *     variances: from the same staged doubles, X's in the workgroups with b == 0, Y's in those with a == 0: a thread adds the
 *     squares of the rows rr, rr + 4, ... (rr = 0..3) of its column by fma in row order, the four threads of a column are added
 *     in the order of rr, the slabs in slab order, one division by N (no E[x^2] - mean^2);
 *     the finishing launch adds the slabs' partials in slab order and divides by N.
 *   Additions at most on a term's way
 *     to a mean:                A_mean(N)   = mrows + mslabs
 *     to a variance:            A_var(N, D) = 8 per + 4 + slabs
 *     to a covariance entry:    A_cov(N, D) = 32 per + slabs     (4 per matrix instruction, 8 instructions per 32 rows, the slabs)
 *   ws: msn_cross_cov_workspace_bytes = 8 (2 mslabs D + 2 slabs D + 4096 slabs pairs) bytes.
 *
 * Forward (two launches, D^2 work, never touches X or Y): from var_x, var_y, cov it writes corr (D x D), comp (2 doubles) =
 *   (on, off), loss (1 float) = on + lambd off rounded once from fp64, M_x = A^T and M_y = A (D x D: both backward products read
 *   their matrix row-major along the inner index), d_x, d_y (D).  One entry per thread and step over blocks = min(ceil(D^2 / 256),
 *   64) workgroups, (c_aa - 1)^2 and c_ab^2 added by fma, the xor tree, the four waves in order, one finishing workgroup likewise:
 *     to on or off:             A_dd(D)     = ceil(D^2 / (256 blocks)) + 9 + ceil(blocks / 256) + 9
 *   r_a and q_b by one thread each, G c added by fma over the D entries of the row or column in index order:
 *     to r_a or q_b:            A_rq(D)     = D
 *   ws: msn_barlow_workspace_bytes = 16 blocks bytes.
 * Backward (one launch): P_x = Yc M_x, P_y = Xc M_y on the same instruction, a 64 x 64 tile of P per workgroup, its fp64
 *   accumulator in registers, the PARTNER's centred rows staged 32 inner columns at a time and M in chunks of 32 x 64 through LDS,
 *     to an entry of P:         A_p(D)      = 32 ceil(D / 32)
 *   dX = fl32(g (P_x + d_x[a] (x_ia - mean_x[a]))), dY = fl32(g (P_y + d_y[b] (y_ib - mean_y[b]))), g a DEVICE float.  Rows past N
 *   are never read and never written (dX, dY have row strides lddx, lddy >= D).
 * No host read anywhere: the step records into a graph.
 * MSN_ERR_SHAPE before any launch: D outside 1..256, N < 2 or >= 2^31, lambd negative or not finite, eps not finite or <= 0, a
 * null pointer, a misaligned pointer, a row stride below D, a workspace that is too small (the queries return 0 for a refused
 * shape). */
size_t msn_cross_cov_workspace_bytes(int64_t N, int D);
int msn_cross_cov(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, double* mean_x, double* mean_y,
                  double* var_x, double* var_y, double* cov, void* ws, size_t ws_bytes, msn_stream_t stream);
size_t msn_barlow_workspace_bytes(int D);
int msn_barlow_fwd(const double* var_x, const double* var_y, const double* cov, int64_t N, int D, double lambd, double eps,
                   float* loss, double* comp, double* corr, double* M_x, double* M_y, double* d_x, double* d_y, void* ws,
                   size_t ws_bytes, msn_stream_t stream);
int msn_barlow_bwd(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, const double* mean_x,
                   const double* mean_y, const double* M_x, const double* M_y, const double* d_x, const double* d_y, const float* g,
                   float* dX, int64_t lddx, float* dY, int64_t lddy, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The sums of centred kernel alignment, CKA (Kornblith et al. 2019; the debiased minibatch form of Nguyen et al. 2021 with the
 * HSIC estimator of Song et al. 2012) (embedding_metrics.py: hsic_sums, cka, CKA; csrc/cka.hip).  X (N, Dx), Y (N, Dy) fp32 with
 * row strides >= D, 4-byte aligned, rows are partners; 2 <= N < 2^31, 1 <= Dx, Dy <= 1024 (they may differ).  Everything is fp64
 * on the device, enqueue only, no atomics, no fills, no zeroed scratch, no host read; every load of X and Y is a 4-byte load, so
 * the bits depend on the values, N, Dx, Dy only (not on stride, alignment or run).  Rows past N are never read.  Non-finite inputs
 * are not checked and propagate.  Neither N x N matrix is written.
 *
 * xc, yc: the rows with the column means subtracted in fp64 ((double)x - mean, one rounding).  kernel 0 (linear): K_ij = xc_i . xc_j;
 * kernel 1 (RBF): K_ij = exp(-d2_ij inv2s2_x), d2_ij = max(0, n_i + n_j - 2 xc_i . xc_j), n_i = |xc_i|^2, inv2s2 = 1 / (2 sigma^2);
 * L likewise over Y.  sigma_x, sigma_y > 0 are used as given; 0 derives sigma^2 = sigma_scale^2 (2 / (N - 1)) sum_i n_i, the mean
 * of d2 over i != j, on the device (equal rows: the sum is 0, inv2s2 is inf, and the set's sums are NaN).  The linear kernel
 * ignores the three.  With rK_i = sum_j K_ij:
 *   out[c][0 .. 7] = KL = sum_ij K_ij L_ij, KK, LL, rKL = sum_i rK_i rL_i, rKK, rLL, sK = sum_i rK_i, sL
 * c = 0 over i != j, c = 1 with the diagonal K_ii = n_i (linear) or exactly 1 (RBF), from the row norms, never from d2.
 *
 * The plan, a function of N alone:
 *   mrows = max(64, ceil(N / 64)), mslabs = ceil(N / mrows);  nparts = ceil(N / 256);
 *   T = ceil(N / 64), per = max(2, ceil(T / ceil(1024 / T))), slabs = ceil(T / per).
 * Launches (five, RBF six): column sums over slabs of mrows rows in row order; means (the slabs in order, / N); one thread per row
 * adds (x - mean)^2 by fma in column order and its workgroup's sum goes to a partial; (RBF) one workgroup adds the partials and
 * writes inv2s2; workgroup (ti, slab) of 256 threads visits the 64 x 64 tiles tj = slab per .. in order, stages the centred rows of
 * both tiles 32 columns at a time (zeros past D and past N) and runs v_mfma_f64_16x16x4_f64 into one accumulator set for X and a
 * second for Y, then finishes the 16 pairs of a lane (i == j, i >= N, j >= N skipped): K L, K K, L L by fma, the row sums over the
 * 16 lanes of a row by xor shuffles 8, 4, 2, 1, rows accumulated over tj in order; one finishing workgroup (thread u owns the rows
 * u, u + 256, ...) adds the slabs of a row in slab order and forms everything else.
 *   Additions at most on a term's way
 *     to a mean:                          A_mean      = mrows + mslabs
 *     to a norm n_i:                      A_norm(D)   = D
 *     to the sum of the norms (sigma):    A_sigma     = 9 + ceil(nparts / 256) + 9
 *     to a dot product xc_i . xc_j:       A_dot(D)    = 32 ceil(D / 32)
 *     of a K_ij to a row sum rK_i:        A_row       = 2 + 4 + per + 1 + slabs + 1    (the last one adds the diagonal)
 *     of a K_ij L_ij to KL (KK, LL):      A_scalar    = 16 per + 9 + ceil(T slabs / 256) + 9 + 1    (the last one: the diagonal's sum)
 *     of a row's term to rKL .. sL and to the diagonal's sums:   A_finish = ceil(N / 256) + 9
 *   ws: msn_hsic_workspace_bytes = 8 (mslabs (Dx + Dy) + (Dx + Dy) + 2 N + 2 nparts + 2 + 2 slabs N + 3 T slabs) bytes.
 * MSN_ERR_SHAPE before any launch: Dx or Dy outside 1..1024, N < 2 or >= 2^31, a row stride below D, an unknown kernel, a negative
 * or non-finite sigma, sigma_scale not finite and > 0, a null or misaligned pointer, a workspace that is too small (the query
 * returns 0 for a refused shape). */
size_t msn_hsic_workspace_bytes(int64_t N, int Dx, int Dy);
int msn_hsic_sums(const float* X, int64_t ldx, int Dx, const float* Y, int64_t ldy, int Dy, int64_t N, int kernel, double sigma_x,
                  double sigma_y, double sigma_scale, double* out, void* ws, size_t ws_bytes, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Threshold-free classification metrics (metrics.py; csrc/rank_metrics.hip): one-vs-rest AUROC, average precision, binned
 * ROC / precision-recall curves and top-k accuracy from integer counts.  Shared by the four entry points: S (N, C) fp32
 * scores with row stride ld >= C, 4-byte aligned (every load of S is a 4-byte load: the bits do not depend on stride or
 * alignment); y int64 (N); a row whose target lies outside [0, C) -- -100 is the usual such value -- is ignored everywhere:
 * neither a positive nor a negative of any class.  Comparisons are IEEE fp32 compares: -0.0 == 0.0, infinities are ordered,
 * and a NaN score compares false both ways (it lies above nothing and at-or-above nothing, itself included: a row whose own
 * score is NaN has p_ge = 0 and turns its class's ap_sum into nan; under msn_threshold_counts it reaches no threshold; under
 * msn_topk_ranks a NaN target score gives rank 0).  1 <= N < 2^31, 1 <= C <= 1024, 1 <= T <= 1024, else MSN_ERR_SHAPE before
 * any launch.
 *
 * Pair counts: for every valid row i with c = y_i and s = S[i, c], over all valid rows j,
 *   counts[i] = {n_gt, n_ge, p_ge} = {#(y_j != c, S[j, c] > s), #(y_j != c, S[j, c] >= s), #(y_j == c, S[j, c] >= s)}
 * (int32 (N, 3); p_ge counts i itself; ignored rows get zeros), and per class
 *   istats[c] = {P_c, Nneg_c, U2_c} (int64 (C, 3)), U2_c = sum_{y_i = c} (2 Nneg_c - n_gt[i] - n_ge[i]),
 *   ap_sum[c] = sum_{y_i = c} p_ge[i] / (p_ge[i] + n_ge[i]) (fp64 (C); each quotient rounded once),
 * so that AUROC_c = U2_c / (2 P_c Nneg_c) (Mann-Whitney, ties at one half) and AP_c = ap_sum[c] / P_c (all positives at one
 * score share one precision: scikit-learn's rule) on the host.  O(N^2) compares; per-slab int32 partials sit in `ws`
 * (msn_rank_counts_workspace_bytes = 12 N slabs bytes) and a second launch finishes: no atomics on memory, no fills, no
 * flags.  counts and istats are integers, so they do not depend on how the rows are cut; ap_sum is added in an order that is
 * a function of N alone (thread t of 1024 adds its rows t, t + 1024, ... in order, 0.0 for a row of another class; then the
 * fixed-order block combine).  Everything repeats bit for bit. */
size_t msn_rank_counts_workspace_bytes(int64_t N, int C);
int msn_rank_counts(const float* S, int64_t ld, const int64_t* y, int64_t N, int C, int* counts, int64_t* istats,
                    double* ap_sum, void* ws, size_t ws_bytes, msn_stream_t stream);
/* Binned curves: thr T ascending fp32 thresholds (DEVICE); acc int64 (C, T, 2) and tot int64 (C, 2), caller-owned DEVICE
 * accumulators over calls (as msn_confusion_matrix's cm):
 *   acc[c, t, 0] += #(i valid, y_i == c, S[i, c] >= thr[t])      acc[c, t, 1] += #(i valid, y_i != c, S[i, c] >= thr[t])
 *   tot[c] += {P_c, Nneg_c}
 * One launch; integer adds only (per-workgroup histogram in LDS over the number of thresholds <= s, suffix sums, one add per
 * non-zero cell), so the result does not depend on their order. */
int msn_threshold_counts(const float* S, int64_t ld, const int64_t* y, int64_t N, int C, const float* thr, int T,
                         int64_t* acc, int64_t* tot, msn_stream_t stream);
/* rank[i] = #(c' : S[i, c'] > S[i, y_i], or S[i, c'] == S[i, y_i] and c' < y_i) per valid row -- among equal scores the
 * lower class comes first, the arg-max rule of msn_cross_entropy_fwd -- into rank_or_null (int32 (N), -1 for ignored rows),
 * and hist[rank[i]] += 1 into a caller-owned int64 (C) DEVICE accumulator: top-k accuracy for every k is a prefix sum of hist.
 * One launch, integer adds only. */
int msn_topk_ranks(const float* S, int64_t ld, const int64_t* y, int64_t N, int C, int* rank_or_null, int64_t* hist,
                   msn_stream_t stream);
/* out[i, c] = x[i, c] - logsumexp(x[i, :]) in fp32, x (N, C) row stride ldx, out row stride ldo, one launch: logits as
 * log-probabilities for ranking (per column monotone in the softmax, across rows).  Evaluated as (x - m) - log1p(t) with m
 * the row maximum and t the sum of exp(x_c - m) over every column but the first maximal one (expf / log1pf of the device
 * library): no rounding at the logits' magnitude.  A row's bits depend on the row and C only.  out must not overlap x. */
int msn_log_softmax_rows(const float* x, int64_t ldx, int64_t N, int C, float* out, int64_t ldo, msn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Calibration of classifier probabilities (calibration.py; csrc/calibration.hip): expected calibration error, reliability
 * diagram and Brier score from integer counts, and the objective of temperature scaling (Guo et al. 2017).  Shared by the
 * entry points, as above: S / P (N, C) fp32 with row stride ld >= C, 4-byte aligned (every load is a 4-byte load: the bits do
 * not depend on stride or alignment); y int64 (N); a row whose target lies outside [0, C) is ignored everywhere.
 * 1 <= N < 2^31, 1 <= C <= 1024, 1 <= B <= 1024, beta finite and > 0, else MSN_ERR_SHAPE before any launch.  No float atomics,
 * no fills, no flags; everything repeats bit for bit.
 *
 * out[i, :] = softmax(beta x[i, :]), the sibling of msn_log_softmax_rows (beta = 1 / T applies a fitted temperature in the same
 * launch): evaluated in fp64 -- t = beta (double)x, m the row maximum, e = exp(t - m), the sum of e in column order, e / sum --
 * and rounded to fp32 once.  A row's bits depend on the row, C and beta only.  A row that holds a NaN or +inf comes out all
 * NaN.  out must not overlap x. */
int msn_softmax_rows(const float* x, int64_t ldx, int64_t N, int C, double beta, float* out, int64_t ldo, msn_stream_t stream);
/* Binned calibration statistics of probabilities P, all integers.  acc int64 (slots, B, 3), slots = 1 (classwise = 0) or 1 + C,
 * and tot int64 (3): caller-owned DEVICE accumulators over calls (as msn_threshold_counts has them).
 * A row with a target in range is VALID when every P[i, c] lies in [0, 1] (a NaN does not; -0.0 does) and the fp64 sum of the
 * row, added in column order, lies within 2^-10 of 1; otherwise it is a BAD row and counts nowhere except tot[1].
 * Fixed point: q(p) = rint((double)p 2^32), ties to even -- the product is exact, so q is an integer in [0, 2^32] that depends
 * on the fp32 bits of p only -- and the bin of p is min(B - 1, (q(p) B) >> 32): integer arithmetic, edges k / B, p = 1 in the
 * last bin.  Slot 0 is the top label: conf = P[i, a], a the first maximal column (the arg-max rule of msn_cross_entropy_fwd),
 * hit = (a == y_i); slot 1 + c (classwise): conf = P[i, c], hit = (y_i == c).  Per valid row and slot, b the bin of conf:
 *   acc[s, b, 0] += 1      acc[s, b, 1] += hit      acc[s, b, 2] += q(conf)
 *   tot[0] += #valid       tot[1] += #bad           tot[2] += rint(brier_i 2^30),  brier_i = sum_c (P[i, c] - [y_i == c])^2
 * with brier_i formed in fp64 in column order, product and add rounded apart (d = (double)p - t; s = s + d d, no contraction).
 * The sum rule bounds brier_i by about 2.002 (< 2^32 in units of 2^-30), q <= 2^32 and N < 2^31: every accumulated sum stays
 * below 2^63.  Being integers, the outputs do not depend on the order of the adds or on how an epoch is cut into batches or
 * ranks, and a SUM all-reduce is exact; the quantisation moves ECE by at most 2^-33.  One launch: per-workgroup histogram in
 * LDS (count, hits, 64-bit sum of q) over a group of slots, one 64-bit integer add per non-zero cell; classwise = 0 reads and
 * bins for slot 0 only. */
int msn_calibration_counts(const float* P, int64_t ld, const int64_t* y, int64_t N, int C, int B, int classwise, int64_t* acc,
                           int64_t* tot, msn_stream_t stream);
/* The objective of temperature scaling and its first two derivatives in beta = 1 / T, fp64:
 *   out = double[5] = {n_valid, sum nll_i, sum g_i, sum h_i, n_bad}  (DEVICE; overwritten, not accumulated)
 * over the rows with a target in range; one that holds a NaN or an infinite logit is BAD: it goes to n_bad and nowhere else.
 * Per valid row, with d_c = (double)x_c - max_c x_c and u = beta d:  p = softmax(u),
 *   nll_i = log(sum_c exp(u_c)) - u_y      g_i = sum_c p_c (x_c - x_y) (= E_p[x] - x_y; exact differences and products, a pair sum)
 *   h_i = sum_c p_c (d_c - mu)^2, mu = g_i + d_y (= Var_p[x], the two-pass form: never negative).
 * The sums over rows run in an order that is a function of N alone -- row i belongs to thread i % 256 of workgroup
 * (i / 256) % min(ceil(N / 256), 512), a thread adds its rows in ascending order, a workgroup combines its threads by the xor
 * tree and then wave by wave, per-workgroup partials in `ws` (msn_temperature_nll_workspace_bytes = 64 bytes per workgroup),
 * and a finishing launch adds them the same way -- and each is carried as a pair (sum, error of the sum: two-sum) that is
 * rounded once at the end, so the three sums are the correctly rounded sums of the rows' terms up to 2^-100.  The bits depend
 * on the rows, N, C and beta only. */
size_t msn_temperature_nll_workspace_bytes(int64_t N);
int msn_temperature_nll(const float* S, int64_t ld, const int64_t* y, int64_t N, int C, double beta, double* out, void* ws,
                        size_t ws_bytes, msn_stream_t stream);

/* feat[r] = (x[r]*m, t[r]*inv_norm*m, m, 0), m = mask[r]: the 4 input channels of the build-defined 1-D CNN
 * encoder for light curves / spectra (value, normalised time / wavelength, validity, pad). */
int msn_series_features(const float* x, const float* t, const uint8_t* mask, int64_t rows, float inv_norm,
                        float* feat, msn_stream_t stream);

/* Build-defined ViT image encoder (not in the reference; fills its `image_encoder` slot):
 * tok[b][0] = cls + pos[0], tok[b][1+i] = patch[b][i] + pos[1+i]  with T = 1 + n_patches, and the
 * compaction dpatch[b][i] = dtok[b][1+i] used by the backward. */
int msn_vit_tokens_fwd(const float* patch, const float* cls, const float* pos, int64_t B, int T, int e,
                       float* tok, msn_stream_t stream);
int msn_vit_tokens_bwd(const float* dtok, int64_t B, int T, int e, float* dpatch, msn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MSN_HIP_H */
