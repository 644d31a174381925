/*
 * gnn_layers.h — fused epilogue of the GraphSAGE / GCN convolution (libgnn_spmm.so).
 *
 * Replaces the elementwise tail of GraphSageConvolution.forward (models.py:18-25) and
 * GraphConvolution.forward (models.py:58-64), plus the dropout GraphSage/GCN apply to each
 * layer's output (models.py:43,82):
 *     h   = cat([hB + biasB, hW + biasW], 1)      (GCN: h = hW + biasW, D1 = 0)
 *     o   = elu(h)
 *     y   = (o - mean(o)) * scale * rsqrt(var(o) + 1e-9) + offset     (biased var, per row)
 *     out = dropout(y, p)                          (training only; inverted scaling)
 * in ONE pass over the rows (one wave per row, the row held in registers), and its
 * backward in one more pass plus a deterministic column reduction for d(scale), d(offset)
 * and the linear biases' gradients d(biasB), d(biasW) (hB / hW are the bias-free linear
 * outputs; biases may be NULL, then their gradients are not written).
 * Dropout masks come from a counter-based hash of (seed, row * D + col): nothing is stored,
 * backward regenerates them.
 *
 * All pointers are device pointers; row strides in elements; D = D1 + D2, D1 % 4 == 0,
 * D <= 2048. Returns 0 or a non-zero status (text: gnn_last_error()).
 */
#ifndef GNN_LAYERS_H
#define GNN_LAYERS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int gnn_sage_norm_fwd_f32(const float* hB, int64_t ldb, int64_t D1, const float* hW, int64_t ldw, int64_t D2,
                          const float* biasB, const float* biasW, const float* scale, const float* offset, int64_t M,
                          float p_drop, uint64_t seed, int training, float* Y, int64_t ldy, float* mean_out,
                          float* rstd_out, void* stream);

size_t gnn_sage_norm_bwd_workspace_bytes(int64_t M, int64_t D);

int gnn_sage_norm_bwd_f32(const float* gY, int64_t ldg, const float* hB, int64_t ldb, int64_t D1, const float* hW,
                          int64_t ldw, int64_t D2, const float* biasB, const float* biasW, const float* scale,
                          const float* mean, const float* rstd, int64_t M, float p_drop, uint64_t seed, int training,
                          float* dhB, float* dhW, float* dscale, float* doffset, float* dbiasB, float* dbiasW,
                          void* workspace, size_t workspace_bytes, void* stream);

/* gnn_sage_norm_bwd_f32 whose output gradient is not a dense gY but the aggregation of the layer
 * above, computed per row as the tail reads it:
 *   gY[r] = Σ_e t_val[e] · G[t_col[e]]  (e over Aᵀ's row r, a C fmaf chain from 0 in CSR order)
 *           + R[rmap[r]]               (when rmap[r] >= 0; rmap NULL: no residual)
 * — the same values gnn_spmm_csr_f32_ex produces for this operand with its row kernel (one wave
 * per row), bit for bit. Replaces the backward aggregation of the top layer (custom_sparse_ops.py:
 * 33-37, A.t().coalesce() @ G, and GraphSAGE's x[sampled] gradient scatter) when Aᵀ's rows are
 * short: the 35 MB gradient is never written nor read back. G and R: 16-byte aligned rows of at
 * least D floats. */
int gnn_sage_norm_bwd_agg_f32(const int32_t* t_rowptr, const int32_t* t_col, const float* t_val, const float* G,
                              int64_t ldG, const float* R, int64_t ldr, const int32_t* rmap, const float* hB,
                              int64_t ldb, int64_t D1, const float* hW, int64_t ldw, int64_t D2, const float* biasB,
                              const float* biasW, const float* scale, const float* mean, const float* rstd, int64_t M,
                              float p_drop, uint64_t seed, int training, float* dhB, float* dhW, float* dscale,
                              float* doffset, float* dbiasB, float* dbiasW, void* workspace, size_t workspace_bytes,
                              void* stream);

/* What the backward (agg = 0: gnn_sage_norm_bwd_f32, 1: gnn_sage_norm_bwd_agg_f32) launches for M
 * rows of width D, for tests and tools that must know which kernel a shape reaches:
 *   split_rows  1: two waves per row (sage_norm_bwd2_kernel<nv>), 0: one (sage_norm_bwd_kernel<nv>)
 *   nv          float4 per lane of that kernel (of half a row in the split form)
 *   grid        its workgroups = the partial rows the finalize kernel sums (1 at M = 0, where
 *               nothing is launched)
 * A pure host function of its arguments and of GNN_SAGE_BWD1, GNN_SAGE_BWD_GRID (read once per
 * process) and GNN_SAGE_BWD2_GRID(_AGG): no HIP call. The forward runs
 * sage_norm_fwd_kernel<ceil(D / 256)> on ceil(M / 4) workgroups for every shape. Output
 * pointers may be NULL. Non-zero when D is not a multiple of 4 in (0, 2048]. */
int gnn_sage_norm_config(int64_t M, int64_t D, int agg, int* split_rows, int* nv, int* grid);

/* ---------------------------------------------------------------------------------
 * fp32 GEMMs of the layers on gfx950 MFMA (gemm.hip): C[b] = A[b] · B[b] for b < nbatch
 * (1..4 problems of one shape in one launch; A, B, C are HOST arrays of device pointers).
 *   A(m, k) = a_kmajor ? A[k*lda + m] : A[m*lda + k]      (M x K)
 *   B(k, n) = b_kmajor ? B[k*ldb + n] : B[n*ldb + k]      (K x N)
 *   C(m, n) = C[m*ldc + n]                                 (M x N, row-major)
 * Replaces the torch.nn.Linear products of GraphSageConvolution / GraphConvolution
 * (models.py:18-21, 58-61) and their backward: forward X·Wᵀ (0, 0), input gradient G·W
 * (0, 1), weight gradient Gᵀ·X (1, 1). Exact fp32 (each output a k-ordered fmaf chain per
 * k-split; splits added in order: deterministic). lda, ldb even and A, B 8-byte aligned
 * (16-byte loads when lda/ldb are multiples of 4 and the pointers 16-byte aligned). When gnn_gemm_f32_workspace_bytes(M, N, K, nbatch) > 0 the k dimension is split
 * and `workspace` must hold that many bytes of device memory.
 * ------------------------------------------------------------------------------- */
size_t gnn_gemm_f32_workspace_bytes(int64_t M, int64_t N, int64_t K, int nbatch);
int gnn_gemm_f32(int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, int nbatch, const float* const* A,
                 int64_t lda, const float* const* B, int64_t ldb, float* const* C, int64_t ldc, void* workspace,
                 size_t workspace_bytes, void* stream);

/* The same contract on the bf16 matrix cores ("split3", gemm.hip): every fp32 operand is cut
 * EXACTLY into three bf16 pieces by truncation (x = h + m + l) and each output accumulates in
 * fp32 the six largest piece products h·h + h·m + m·h + h·l + m·m + l·h per k (each exact in
 * fp32); the dropped products are below 3·2^-24·|a||b|, i.e. fp32-level accuracy (bounded
 * against fp64 by the same tolerance as gnn_gemm_f32 in tests/test_gemm_gpu.py), at 2.67x the
 * f32-input matrix rate. Deterministic (fixed accumulation order, k-splits added in order). */
size_t gnn_gemm_f32_split3_workspace_bytes(int64_t M, int64_t N, int64_t K, int nbatch);
int gnn_gemm_f32_split3(int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, int nbatch,
                        const float* const* A, int64_t lda, const float* const* B, int64_t ldb, float* const* C,
                        int64_t ldc, void* workspace, size_t workspace_bytes, void* stream);

/* gnn_gemm_f32_split3 with row-indexed operands: row m of an m-major A is A[ia[b][m]] (a_rows
 * source rows), row k of a k-major B is B[ib[b][k]] (b_rows source rows); ia / ib or entries NULL
 * = not indexed (an indexed k-major A or m-major B is rejected). Bit-identical to the split3
 * product of the gathered operands — GraphSAGE's x[sampled] (models.py:18-21) read in place. */
int gnn_gemm_f32_split3_indexed(int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, int nbatch,
                                const float* const* A, int64_t lda, const int64_t* const* ia, int64_t a_rows,
                                const float* const* B, int64_t ldb, const int64_t* const* ib, int64_t b_rows,
                                float* const* C, int64_t ldc, void* workspace, size_t workspace_bytes, void* stream);

/* The split kernel at a chosen piece count: the opt-in reduced-precision modes. fp32 operands and
 * fp32 accumulation as above, fewer mantissa bits on the matrix-core operands. Every operand element
 * x is replaced by a rounded x', and each output accumulates in fp32 the EXACT bf16 x bf16 products
 * of the kept pieces, in split3's order:
 *   pieces = 3 ("split3"): the entry points above, bit for bit.
 *   pieces = 2 ("split2"): h = trunc_bf16(x) (split3's own h), r = x - h (exact), m = RNE_bf16(r);
 *     x' = h + m, |x - x'| <= 2^-15 |x|. Per k step the four products m·m, m·h, h·m, h·h — split3's
 *     list l·h, m·m, h·l, m·h, h·m, h·h without the two l products — i.e. the fp32-accumulated
 *     product of the rounded operands (h + m)(h + m): no dropped cross term.
 *   pieces = 1 ("bf16"): h = RNE_bf16(x) (round to nearest even, torch's x.bfloat16()); x' = h,
 *     |x - x'| <= 2^-8 |x|. One product h·h per k step.
 * For every output and k split, k runs ascending in steps of 16, one MFMA per piece product per
 * step; the k-split count, the tail-tile plan, the tile map and the workspace are split3's for the
 * same shape and batch count (at its 128 x 128 tile: GNN_GEMM_WIDE is ignored below 3 pieces). So
 * on operands that already fit the kept pieces (<= 8 significant bits for bf16, <= 16 for split2)
 * a reduced mode reproduces split3 bit for bit: the removed products are all ±0. Inputs below
 * 2^-100 in magnitude, NaN and Inf are unspecified, as for split3. pieces outside 1..3: status -22
 * before any device call (the workspace query returns 0). Operands of >= 2 GiB are refused below 3
 * pieces. The indexed form is gnn_gemm_f32_split3_indexed's, bit-identical to the same mode's
 * product of the gathered operands. */
size_t gnn_gemm_f32_split_workspace_bytes(int pieces, int64_t M, int64_t N, int64_t K, int nbatch);
int gnn_gemm_f32_split(int pieces, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, int nbatch,
                       const float* const* A, int64_t lda, const float* const* B, int64_t ldb, float* const* C,
                       int64_t ldc, void* workspace, size_t workspace_bytes, void* stream);
int gnn_gemm_f32_split_indexed(int pieces, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, int nbatch,
                               const float* const* A, int64_t lda, const int64_t* const* ia, int64_t a_rows,
                               const float* const* B, int64_t ldb, const int64_t* const* ib, int64_t b_rows,
                               float* const* C, int64_t ldc, void* workspace, size_t workspace_bytes, void* stream);

/* split3 over operands split ONCE into their three bf16 pieces ("p3"): gnn_gemm_p3_pack_f32 writes
 * an operand viewed as R rows (M for A, N for B) by K — element (r, k) = src[row(r)*ld + k]
 * (kmajor = 0) or src[row(k)*ld + r] (kmajor = 1), row() through idx when given — as three
 * zero-padded planes [piece][k tile of 16][R rounded up to 128][16] bf16
 * (gnn_gemm_p3_packed_bytes(R, K) bytes, 16-byte aligned); gnn_gemm_p3 then computes
 * C[b] (M x N, row stride ldc) = A[b] · B[b]ᵀ-as-packed with the split3 kernel's tile, k steps
 * and MFMA order: bit-identical to gnn_gemm_f32_split3 on the same operands for shapes without
 * split3's tail tiles (gnn_gemm_f32_split3 sums the last 1-32 tiles past a multiple of 256 as k
 * pieces when GNN_GEMM_TAIL is on; p3 has no tail mode — equal there with GNN_GEMM_TAIL=0). */
size_t gnn_gemm_p3_packed_bytes(int64_t R, int64_t K);
int gnn_gemm_p3_pack_f32(const float* src, int64_t ld, int kmajor, const int64_t* idx, int64_t R, int64_t K,
                         void* out, size_t out_bytes, void* stream);
size_t gnn_gemm_p3_workspace_bytes(int64_t M, int64_t N, int64_t K, int nbatch);
int gnn_gemm_p3(int64_t M, int64_t N, int64_t K, int nbatch, const void* const* Ap, const void* const* Bp,
                float* const* C, int64_t ldc, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Classifier head + loss (head.hip). Replaces GNN.forward's tail (models.py:90-97:
 * F.normalize(x, 2, 1) -> dropout(p) -> nn.Linear(D, C)) and utils.loss with sigmoid_loss
 * (utils.py:129-140: BCEWithLogitsLoss(weight = 1/M per row, reduction "sum")):
 *   xd = dropout(x / max(||x||, 1e-12))  -> stored M x D (row stride D) for dW = dzᵀ·xd
 *   z  = xd·Wᵀ + bias                    -> stored M x C (logits)
 *   *loss = Σ_rows Σ_j (max(z,0) - z y + log1p(exp(-|z|))) / M   (rows summed in fixed order)
 * norm[M] = ||x|| per row, rowloss[M] = the per-row terms (workspace). W is C x D row-major
 * (nn.Linear.weight), labels M x C with row stride ldl; bias may be NULL. D % 4 == 0,
 * D <= 2048, C <= 256; X, W, xd 16-byte aligned. Dropout: the counter hash of (seed, r*D+c)
 * (as gnn_sage_norm_*), training = 0 or p = 0 disables it.
 * Backward: dz = (*grad_loss) (sigmoid(z) - y) / M (M x C, written for dW / db), and
 * dX = d/dx of the normalisation applied to mask · (dz·W). grad_loss may be NULL (1).
 * ------------------------------------------------------------------------------- */
int gnn_head_bce_fwd_f32(const float* X, int64_t ldx, int64_t M, int64_t D, const float* W, const float* bias,
                         int64_t C, const float* labels, int64_t ldl, float p, uint64_t seed, int training,
                         float* xd, float* z, float* norm, float* rowloss, float* loss, void* stream);
int gnn_head_bce_bwd_f32(const float* X, int64_t ldx, int64_t M, int64_t D, const float* W, int64_t C,
                         const float* labels, int64_t ldl, const float* grad_loss, float p, uint64_t seed,
                         int training, const float* z, const float* norm, float* dz, float* dX, int64_t lddx,
                         void* stream);

/* The same head with the softmax cross-entropy loss (utils.py:138-140, sigmoid_loss = False:
 * CrossEntropyLoss(reduction "none") over float target rows, weighted 1/M and summed):
 *   lse_r = m_r + log Σ_j exp(z_rj - m_r), m_r = max_j z_rj       -> stored lse[M] for the backward
 *   *loss = Σ_rows Σ_j y_rj (lse_r - z_rj) / M   (subtracted per class; rows summed in fixed order)
 * The row pass, the dropout hash and the seed are those of gnn_head_bce_fwd_f32: xd, z and norm
 * are bit-identical to what it writes for the same inputs. The targets are probabilities, as in
 * torch: a row need not sum to 1, and an all-zero row contributes 0. Same contract (D % 4 == 0,
 * D <= 2048, C <= 256, 16-byte rows, labels M x C with row stride ldl). No atomics: deterministic.
 * Backward: dz = (*grad_loss) (exp(z - lse) Σ_j y_j - y) / M, then dX as in the BCE backward. */
int gnn_head_ce_fwd_f32(const float* X, int64_t ldx, int64_t M, int64_t D, const float* W, const float* bias,
                        int64_t C, const float* labels, int64_t ldl, float p, uint64_t seed, int training, float* xd,
                        float* z, float* norm, float* rowloss, float* loss, float* lse, void* stream);
int gnn_head_ce_bwd_f32(const float* X, int64_t ldx, int64_t M, int64_t D, const float* W, int64_t C,
                        const float* labels, int64_t ldl, const float* grad_loss, float p, uint64_t seed, int training,
                        const float* z, const float* norm, float* dz, float* dX, int64_t lddx, const float* lse,
                        void* stream);

/* The head's bias gradient db[c] = Σ_rows dz[r][c] (dz M x C, row stride C) in a fixed order: one
 * workgroup per class, each thread a strided set of rows, then a fixed tree — the kernel the native
 * step (gnn_train_step_f32) runs for it, so the Python fused path (fused.HeadBCEFn / HeadCEFn) and
 * the native step give the same bits, where a library reduction's order is its own. M = 0 writes
 * zeros; C = 0 launches nothing. */
int gnn_head_bias_grad_f32(const float* dz, int64_t M, int64_t C, float* db, void* stream);

/* Evaluation head (head.hip): the forward above with training = 0 for a validation / test batch
 * (main.py:178-199, 217-241: model.eval(), forward, utils.loss, utils.calc_f1) — no dropout, no
 * xd / norm stores — plus the per-class prediction counts utils.calc_f1 (utils.py:142-149) feeds
 * to sklearn's f1_score, so neither logits nor labels leave the device:
 *   z (M x C, row stride ldz; NULL: not written): the same dot products in the same order as
 *     gnn_head_bce_fwd_f32, bit-identical to its logits with training = 0;
 *   *loss: the same terms and the same fixed-order row sum, bit-identical too;
 *   counts[3][C] (int32, overwritten): tp, fp, fn per class over the M rows.
 *     mode 0 (is_sigmoid = True):  pred_j = z_j > 0, true_j = y_j > 0.5 per class;
 *     mode 1 (is_sigmoid = False): pred = argmax_j z_j, true = argmax_j y_j (the first index wins
 *       ties, as np.argmax); tp[c] = #(pred = c and true = c), fp[c] = #(pred = c, true != c),
 *       fn[c] = #(true = c, pred != c).
 *     One deviation in mode 0: the reference thresholds sigmoid(z) > 0.5 computed in fp32, which
 *     differs from z > 0 only for 0 < z < ~1.2e-7, where the fp32 sigmoid rounds to exactly 0.5
 *     (there the reference predicts 0, this kernel 1).
 * Two launches: the row pass leaves each row's loss terms in rowloss[M] and its predicted / true
 * class sets as bit masks in rowmask[M][8] (uint64; words 0-3 predicted, 4-7 true); one workgroup
 * per class then counts its bit over the rows (integers: exact and deterministic, no atomics)
 * and one more sums the loss. labels NULL: only z is produced (predict); loss, counts, rowloss
 * and rowmask are not touched and may be NULL. M = 0 launches no row pass and writes zero counts
 * and a zero loss. Contract as gnn_head_bce_fwd_f32: D % 4 == 0, D <= 2048, C <= 256, X and W
 * 16-byte aligned, ldx % 4 == 0. */
int gnn_head_eval_f32(const float* X, int64_t ldx, int64_t M, int64_t D, const float* W, const float* bias,
                      int64_t C, const float* labels, int64_t ldl, float* z, int64_t ldz, float* rowloss,
                      uint64_t* rowmask, float* loss, int32_t* counts, int mode, void* stream);

/* gnn_head_eval_f32 with the loss chosen by loss_kind: 0 = the BCE-with-logits terms (what
 * gnn_head_eval_f32 computes: it forwards here with kind 0), 1 = the softmax cross-entropy terms of
 * gnn_head_ce_fwd_f32, bit-identical to its loss with training = 0. Logits, masks and counts do
 * not depend on the kind, and mode is independent of it. Any other kind returns a status before
 * anything is launched. */
int gnn_head_eval_loss_f32(const float* X, int64_t ldx, int64_t M, int64_t D, const float* W, const float* bias,
                           int64_t C, const float* labels, int64_t ldl, float* z, int64_t ldz, float* rowloss,
                           uint64_t* rowmask, float* loss, int32_t* counts, int mode, int loss_kind, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GNN_LAYERS_H */
