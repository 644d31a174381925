/* gnn_step.h — native executor of a GraphSAGE / GCN training step's forward + backward
 * (libgnn_spmm.so, gfx950; gnn_amd/csrc/step.hip).
 *
 * Replaces the host side of the reference's step (main.py:122-146: model(x0, adjs,
 * sampled_nodes) -> utils.loss -> loss.backward(); models.py:6-97, utils.py:129-140) — the
 * ~45 autograd Functions / ctypes calls per step of gnn_amd.models' fused path — with ONE call
 * that issues the same kernels (aggregation gnn_spmm_csr_f32[_ex], row gather, split3 / rocBLAS
 * GEMMs, gnn_sage_norm_*, gnn_head_bce_* or gnn_head_ce_*) with the same routing and dropout seeds. Gradients
 * are written into caller-provided buffers; clip / all-reduce / Adam stay with the caller
 * (gnn_optim.h). Stream-ordered; every intermediate lives in one caller-provided workspace of
 * gnn_train_step_workspace_bytes(desc) bytes (256-byte aligned). Returns 0 or a status (text:
 * gnn_last_error()).
 *
 * The descriptor is an int64 array: a header of GNN_STEP_HEADER slots (GNN_SH_*), then
 * GNN_STEP_LAYER_SLOTS slots per layer, bottom-up (GNN_SL_*). Pointers are device pointers
 * stored as integers; float scalars as their IEEE bits.
 *   header: kind (GNN_STEP_SAGE: cat[linearB(x[sampled]), linearW(A·x)]; GNN_STEP_GCN:
 *     linear(A·x)), layers, nhid N, x0 (K0 x F0, row stride ldx0: the staged X0), the head
 *     (W C x D, bias, their gradient buffers), labels (M_top x C, row stride ldl), the head's
 *     dropout seed, p (dropout), training (0: no dropout), loss (device float out), and
 *     optionally timing: a HOST int64 array T, T[0] = capacity in records, then records of
 *     GNN_STEP_TIMING_SLOTS slots; the caller puts a hipEvent_t pair in slots 0-1 of each, and
 *     the step arms them around its aggregation kernels in call order (forward layers bottom-up,
 *     then the backward aggregations top-down) and writes slots 2-15: kind (0 fwd, 1 bwd),
 *     layer, M, K, nnz, F, padded F, ldx, ldy, X, Y (device addresses), residual rows, 1, the
 *     element kind of X (GNN_SL_XKIND);
 *     and optionally gradient-ready events: a HOST int64 array E, E[0] = entries, E[1] = a
 *     hipEvent_t recorded once the head's gradients are final, E[2 + l] = one recorded once
 *     layer l's gradients (weights, biases, scale, offset) are final (0 = none): the caller's
 *     data-parallel exchange starts on a bucket while the backward of the layers below runs;
 *     and optionally a staging gate: a hipEvent_t (GNN_SH_STAGE_EVENT, 0 = none) recorded on the
 *     step's stream right after layer GNN_SH_STAGE_LAYER's forward aggregation — the caller's
 *     staging stream waits on it before the next batches' row gathers and layer extractions, so
 *     those gather-bound kernels run beside the GEMMs and tails instead of competing with the
 *     aggregation for L2 (main.py:129-137's staging, overlapped with the step);
 *     and the phase (GNN_SH_PHASE): 0 = the whole step; 1 = only layer 0's forward aggregation
 *     A_0·x0, into the workspace (a data-parallel caller issues the NEXT batch's while this
 *     step's gradient all-reduce runs: it reads only the batch, never a parameter); 2 = the step
 *     of a batch whose layer-0 aggregation a phase-1 call with the same descriptor already issued
 *     into the same workspace (it is not issued again). 0 and 1 + 2 give the same results.
 *     and the loss kind (GNN_SH_LOSS_KIND): GNN_LOSS_BCE (0, so every descriptor built before the
 *     slot had a meaning) = BCE with logits (utils.loss with sigmoid_loss), GNN_LOSS_CE = softmax
 *     cross-entropy over the float label rows (sigmoid_loss = False); it picks the head's forward /
 *     backward pair (gnn_layers.h) and nothing else. Any other value is refused: both
 *     *_workspace_bytes functions return 0 and neither step function launches anything.
 *   layer l: the operand A (rowptr / col / val, M x K, nnz) and its transpose (K x M, layers >= 1),
 *     sampled (int64 [M], SAGE) and rmap (int32 [K], rmap[sampled[i]] = i, SAGE layers >= 1),
 *     weights W_W / W_B (N x F row-major), biases, scale / offset, their gradient buffers, the
 *     dropout seed. Layer l >= 1 reads layer l-1's output (K_l must equal M_{l-1}).
 *     GNN_SL_XKIND: the element kind of the layer's input (gnn_spmm.h GNN_FEAT_*). 0 = fp32, so
 *     every descriptor built before the slot had a meaning keeps it (GNN_STEP_VERSION stays 1).
 *     GNN_FEAT_F16 / GNN_FEAT_BF16 are allowed on layer 0 only: GNN_SH_X0 is then a 16-bit pointer
 *     (8-byte aligned) and GNN_SH_LDX0 counts elements (a multiple of 4, with room for F0 rounded up
 *     to 4). The layer-0 aggregation reads those rows as they are (gnn_spmm_csr_h16_f32, also in
 *     phase 1; bit-identical to the fp32 call on the widened rows), into rows of F0 rounded up to 4
 *     and then to 32 floats — the stride of the fp32 X0 a feature store stages today, so the
 *     workspace is the widened step's; SAGE's x[sampled] is gathered and widened into the layer's
 *     xs buffer (gnn_gather_rows_h16_f32) for linearB and its weight gradient: the split3 GEMMs do
 *     not read 16-bit rows in place. Any other value, or a non-zero kind on a layer >= 1, is
 *     refused like a bad loss kind: both *_workspace_bytes functions return 0, nothing is launched.
 *     GNN_SL_DENSE: 0 = an aggregating layer (every descriptor built before the slot had a meaning,
 *     so GNN_STEP_VERSION stays 1); 1 = an order-0 layer (the reference's --orders 0, models.py:17-21,
 *     59-60): Y_l = sage_norm(X·W_Wᵀ + b_W). Any other value is refused like a bad loss kind (both
 *     *_workspace_bytes functions return 0, nothing is launched, gnn_last_error() names the layer).
 *     An order-0 layer has no operand: ROWPTR / COL / VAL / NNZ / T* / SAMPLED / NSAMPLED / RMAP are
 *     ignored and may be 0. K must equal M; for l >= 1 that is M_{l-1}, for l = 0 the row count of x0.
 *     SAGE: linearB takes no part, so WB / BB / GWB / GBB are ignored and may be 0 (never written),
 *     and the layer's output is N wide, not 2N: scale / offset have N entries, the layer above reads
 *     F_{l+1} = N and the head D = D_top. GCN: N wide as every layer. All layers may be order 0 (an
 *     MLP). Forward: X is read in place (x0 at ldx0, or the layer below's output), one product routed
 *     as the aggregating layers' pairs (split3 where its tiles fill the chip, else rocBLAS), then the
 *     tail. Backward: for l >= 1 the input gradient dhW·W_W is written straight into layer l-1's
 *     gradient buffer (no transpose, no aggregation); the weight gradient dhWᵀ·X reads X in place.
 *     An aggregating layer above an order-0 layer may still have its backward aggregation folded
 *     into that layer's tail backward; results are bit-identical either way. With GNN_SL_XKIND 16-bit
 *     on an order-0 layer 0 the rows are widened once into the workspace (gnn_gather_rows_h16_f32,
 *     exact) and the layer runs as fp32: bit-identical to the step on the widened x0.
 *     Phases: with an order-0 layer 0 a phase-1 call launches no kernel (it still records the
 *     staging gate if GNN_SH_STAGE_LAYER is 0) and phase 2 issues what phase 0 does; 1 + 2 equals 0
 *     for every mix of orders. The staging gate is recorded exactly once per step: right after layer
 *     GNN_SH_STAGE_LAYER's forward aggregation, or, if that layer is order 0, where the aggregation
 *     would have been issued — before the layer's GEMM. Timing records are written for aggregations
 *     only; the NSAMPLED == M check applies to aggregating SAGE layers only.
 *     GNN_SL_GEMM: the precision of the layer's matrix-core products (gnn_layers.h,
 *     gnn_gemm_f32_split). 0 = as the environment says (GNN_GEMM_ALGO: unset / split3, f32, or the
 *     reduced modes split2 / bf16 process-wide), so every descriptor built before the slot had a
 *     meaning keeps it (GNN_STEP_VERSION stays 1). 1, 2 or 3 = that many bf16 pieces per operand
 *     (1: "bf16", 2: "split2", 3: split3) for every product of the layer that the step routes to the
 *     split kernel: the forward pair, the input gradients, the weight gradients, their row-indexed
 *     forms and their single-product launches under GNN_STEP_OVERLAP. The routing is split3's and
 *     does not depend on the slot; products on the vendor GEMM stay fp32 sgemm, the head is not
 *     touched, the workspace is unchanged, and gnn_eval_step_f32 honours the slot through the shared
 *     forward. Any other value is refused like a bad loss kind (both *_workspace_bytes functions
 *     return 0, nothing is launched, gnn_last_error() names the layer).
 */
#ifndef GNN_STEP_H
#define GNN_STEP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNN_STEP_VERSION 1
#define GNN_STEP_MAX_LAYERS 4
#define GNN_STEP_HEADER 24
#define GNN_STEP_LAYER_SLOTS 32
#define GNN_STEP_SAGE 0
#define GNN_STEP_GCN 1
#define GNN_STEP_TIMING_SLOTS 16
#define GNN_LOSS_BCE 0
#define GNN_LOSS_CE 1

enum {
  GNN_SH_VERSION = 0, GNN_SH_LAYERS = 1, GNN_SH_KIND = 2, GNN_SH_X0 = 3, GNN_SH_LDX0 = 4, GNN_SH_F0 = 5,
  GNN_SH_HEAD_W = 6, GNN_SH_HEAD_B = 7, GNN_SH_HEAD_GW = 8, GNN_SH_HEAD_GB = 9, GNN_SH_CLASSES = 10,
  GNN_SH_LABELS = 11, GNN_SH_LDL = 12, GNN_SH_HEAD_SEED = 13, GNN_SH_PDROP_BITS = 14, GNN_SH_TRAINING = 15,
  GNN_SH_LOSS = 16, GNN_SH_NHID = 17, GNN_SH_TIMING = 18, GNN_SH_GRAD_EVENTS = 19, GNN_SH_STAGE_EVENT = 20,
  GNN_SH_STAGE_LAYER = 21, GNN_SH_PHASE = 22, GNN_SH_LOSS_KIND = 23
};
enum {
  GNN_SL_ROWPTR = 0, GNN_SL_COL = 1, GNN_SL_VAL = 2, GNN_SL_M = 3, GNN_SL_K = 4, GNN_SL_NNZ = 5,
  GNN_SL_TROWPTR = 6, GNN_SL_TCOL = 7, GNN_SL_TVAL = 8, GNN_SL_SAMPLED = 9, GNN_SL_NSAMPLED = 10,
  GNN_SL_RMAP = 11, GNN_SL_WW = 12, GNN_SL_BW = 13, GNN_SL_WB = 14, GNN_SL_BB = 15, GNN_SL_SCALE = 16,
  GNN_SL_OFFSET = 17, GNN_SL_GWW = 18, GNN_SL_GBW = 19, GNN_SL_GWB = 20, GNN_SL_GBB = 21, GNN_SL_GSCALE = 22,
  GNN_SL_GOFFSET = 23, GNN_SL_SEED = 24, GNN_SL_XKIND = 25, GNN_SL_DENSE = 26, GNN_SL_GEMM = 27
};

size_t gnn_train_step_workspace_bytes(const int64_t* desc);
int gnn_train_step_f32(const int64_t* desc, void* workspace, size_t workspace_bytes, void* stream);

/* Forward-only step for validation / test batches (main.py:178-199, 217-241: model.eval(), the
 * same staging and forward, utils.loss, utils.calc_f1): the training step's forward with
 * training = 0 — the same kernels with the same routing, issued by the same code — and then the
 * evaluation head (gnn_head_eval_loss_f32, gnn_layers.h): the loss (of GNN_SH_LOSS_KIND), the logits (M_top x C, row stride
 * ldz; NULL: not written) and the per-class prediction counts[3][C] (tp, fp, fn; int32,
 * overwritten; mode 0: sigmoid / multi-label, 1: argmax / single-label; independent of the loss kind).
 * Takes the same version-1 descriptor and reads only what a forward needs: gradient pointers,
 * transposes (GNN_SL_T*), GNN_SL_RMAP, the seeds, GNN_SH_TRAINING, GNN_SH_TIMING and
 * GNN_SH_GRAD_EVENTS are ignored and may be 0; GNN_SH_PHASE must be 0; GNN_SH_STAGE_EVENT is
 * honoured as in training. GNN_SH_LABELS and GNN_SH_LOSS may be 0 together (predict: only the
 * logits; counts may be NULL). The loss equals, bit for bit, what gnn_train_step_f32 writes for
 * the same descriptor with training = 0.
 * The workspace holds no backward buffer and one set of forward buffers shared by all layers:
 * gnn_eval_step_workspace_bytes(desc) < gnn_train_step_workspace_bytes(desc) for every valid
 * descriptor. It is validated (size, 256-byte alignment) before anything is launched. */
size_t gnn_eval_step_workspace_bytes(const int64_t* desc);
int gnn_eval_step_f32(const int64_t* desc, float* logits, int64_t ldz, int32_t* counts, int mode, void* workspace,
                      size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GNN_STEP_H */
