/*
 * gnn_spmm.h — C ABI of the MI355X-native SpMM-aggregation path (libgnn_spmm.so).
 *
 * This is the drop-in boundary for the reference's CUDA extension `spmm`
 * (reference: spmm_cpp/spmm.cpp:52-56, bound in custom_sparse_ops.py:8). Every entry
 * point takes plain device pointers, sizes and a hipStream_t (passed as void*), launches
 * stream-ordered work only (no host synchronisation, no allocation, graph-capturable),
 * and returns 0 on success or a non-zero status whose text is gnn_last_error().
 *
 * Status codes: 0 = ok; GNN_EINVAL (-22) = bad argument (shape, alignment, workspace);
 * any positive value = the hipError_t of a failed launch.
 *
 * Index types: CSR row pointers and column indices are int32 (the reference narrows its
 * int64 COO indices to int32 too: cuda_spmm.cu:620-621), so M, K and nnz must be < 2^31.
 */
#ifndef GNN_SPMM_H
#define GNN_SPMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNN_EINVAL (-22)

/* Text of the last error raised on the calling thread ("" if none). */
const char* gnn_last_error(void);

/* Library version string (build id). */
const char* gnn_version(void);

/* ---------------------------------------------------------------------------------
 * SpMM forward / backward:  Y[M, F] = A[M, K] · X[K, F]   (fp32, CSR operand)
 *
 * Replaces: spmm_load_balance(sparseMat, denseMat)   spmm_cpp/spmm.cpp:23-27
 *           -> spmm_cuda_v2                           spmm_cpp/cuda_spmm.cu:619-704
 *           and spmm_naive (spmm.cpp:38-42, same math, no load balance).
 * The reference's backward is the same call on A^T (custom_sparse_ops.py:33-37); here the
 * caller passes the CSR of A^T produced by gnn_csr_transpose.
 *
 * X rows are read with stride ldx (elements), Y rows written with stride ldy; F <= ldx,
 * F <= ldy. Every one of the M rows of Y (columns [0, F)) is written (empty rows get 0),
 * so Y needs no zero-fill. Work is cut into units of `unit_nnz` consecutive nonzeros; a row
 * of at most unit_nnz entries is summed whole, in CSR order, by the unit holding its first
 * entry (bit for bit a C fmaf chain); longer rows are summed per unit and their pieces added
 * in unit order by a second kernel — deterministic (bitwise reproducible run to run).
 *
 * `workspace` must hold gnn_spmm_workspace_bytes(M, nnz, F, unit_nnz) bytes (device
 * memory); unit_nnz <= 0 selects gnn_spmm_default_unit_nnz(M, nnz, F).
 * ------------------------------------------------------------------------------- */
int64_t gnn_spmm_default_unit_nnz(int64_t M, int64_t nnz, int64_t F);
size_t gnn_spmm_workspace_bytes(int64_t M, int64_t nnz, int64_t F, int64_t unit_nnz);
int gnn_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                     int64_t M, int64_t K, int64_t nnz,
                     const float* X, int64_t ldx,
                     float* Y, int64_t ldy, int64_t F,
                     void* workspace, size_t workspace_bytes, int64_t unit_nnz,
                     void* stream);

/* Same, plus a row-mapped residual fused into the stores:
 *     Y[r, :] = (A · X)[r, :] + (rmap[r] >= 0 ? R[rmap[r], :] : 0)
 * rmap (int32, M entries, device) may be NULL (then R is ignored). This is the backward of
 * GraphSageConvolution's two inputs (models.py:18-21): d(x) = A^T · d(A·x) + scatter of
 * d(x[sampled]) — the scatter is the residual with rmap = inverse of the sampled-row map.
 * R rows are read with stride ldr (F <= ldr) and must be aligned like Y. */
int gnn_spmm_csr_f32_ex(const int32_t* rowptr, const int32_t* col, const float* val,
                        int64_t M, int64_t K, int64_t nnz,
                        const float* X, int64_t ldx,
                        float* Y, int64_t ldy, int64_t F,
                        const float* R, int64_t ldr, const int32_t* rmap,
                        void* workspace, size_t workspace_bytes, int64_t unit_nnz,
                        void* stream);

/* Describe the kernel configuration gnn_spmm_csr_f32 would pick (vector width, lanes per
 * column group, column chunks per lane, column tiles, units). For diagnostics/benchmarks. */
int gnn_spmm_config(int64_t M, int64_t K, int64_t nnz, int64_t F, int64_t ldx, int64_t ldy,
                    const void* X, const void* Y, int64_t unit_nnz, int32_t out[6]);

/* The name of the main aggregation kernel gnn_spmm_csr_f32(_ex) would launch for this call, as
 * rocprofv3 lists it: "spmm_unit_kernel<VW, G, NJ, U, RES>" (nnz work units + the combine of
 * cut rows) or, for small operands (up to 64 k nonzeros, unit_nnz == 0: the layer-2 calls),
 * "spmm_row_kernel<VW, NJ, U, WPR, RES>" (a workgroup of WPR waves per (row, column slice), no
 * combine launch). residual != 0 names the row-mapped residual variant. */
int gnn_spmm_kernel_name(int64_t M, int64_t K, int64_t nnz, int64_t F, int64_t ldx, int64_t ldy,
                         const void* X, const void* Y, int64_t unit_nnz, int residual, char* out,
                         size_t out_bytes);

/* The same aggregation reading X as 16-bit rows (kind = GNN_FEAT_F16 or GNN_FEAT_BF16, declared
 * with the feature gathers below; ldx in 16-bit elements): Y = A · (float)X without an fp32 copy
 * of X — layer 0 straight from a 16-bit feature store's staged rows. A lane loads 4 elements
 * (8 bytes) where the fp32 kernel loads a float4 and widens them in registers (both conversions
 * exact); lane groups, column tiles, unit size, row / unit kernel choice and workgroup order are
 * those gnn_spmm_csr_f32 takes for the same (M, K, nnz, F) with 4-wide vectors, so Y equals that
 * call's result on the widened X bit for bit. Same contract (stream-ordered, no allocation, no
 * host synchronisation, graph-capturable, timing hook honoured) and same workspace size
 * (gnn_spmm_workspace_bytes). There is no scalar form and no residual: refused with GNN_EINVAL
 * before anything is launched are a kind other than 1 or 2, an X that is not 8-byte aligned, a Y
 * that is not 16-byte aligned, ldx, ldy or F not a multiple of 4, and F > ldx or F > ldy — a
 * caller whose rows do not fit widens them first. */
int gnn_spmm_csr_h16_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                         int64_t M, int64_t K, int64_t nnz,
                         const void* X, int64_t ldx, int kind,
                         float* Y, int64_t ldy, int64_t F,
                         void* workspace, size_t workspace_bytes, int64_t unit_nnz,
                         void* stream);

/* The configuration gnn_spmm_csr_h16_f32 would pick: out[0..5] as gnn_spmm_config (out[0] = 4),
 * out[6] = waves per row of the row kernel (0: the unit kernel), out[7] = 16-bit elements per
 * load. X / Y are read for nothing here (the call itself checks their alignment). */
int gnn_spmm_h16_config(int64_t M, int64_t K, int64_t nnz, int64_t F, int64_t ldx, int64_t ldy,
                        const void* X, const void* Y, int64_t unit_nnz, int32_t out[8]);

/* Aggregation over rows [row0, row0 + rows) of the graph resident on the device (the canonical CSR
 * a LADIES extraction reads, gnn_extract.h: int64 indptr[num_nodes + 1], int32 indices, int32 row
 * degrees), for full-neighbourhood inference:
 *     Y[i, 0:F] = sum over e in [indptr[row0+i], indptr[row0+i+1]) of w_i * X[indices[e], 0:F],
 *     w_i = (float)(1.0 / (double)degree[row0+i])
 * — gnn_build_operand_f32's value with normfact = 1. This is lap[rows, :] · X, the expectation of
 * the operand the reference's sampler draws (sampler.py:113-139: adj = U[:, after_nodes] scaled by
 * 1/(s·p), whose mean over the draw is U = lap[rows, :]); every sampled layer of this project
 * estimates it. X has num_nodes rows (kind GNN_FEAT_F32, or GNN_FEAT_F16 / GNN_FEAT_BF16 rows read as
 * gnn_spmm_csr_h16_f32 reads them; ldx in elements of X); rows of Y are block-local; empty rows
 * store zeros.
 *
 * e0 = indptr[row0] and nnz = indptr[row0 + rows] - e0 are the host's copies (offsets into the
 * graph are int64: the graph may hold 2^31 entries or more, a block may not). One small kernel
 * writes the block's int32 row pointer (indptr[row0+i] - e0, clamped to [0, nnz] with its ends
 * pinned to 0 and nnz, so a device indptr that disagrees with e0 / nnz cannot make the
 * aggregation read outside the block) and its nnz weights into the workspace; the sums are then
 * gnn_spmm_csr_f32 / gnn_spmm_csr_h16_f32 on (that pointer, indices + e0, the weights): the
 * columns are read in place, and kernel choice, launch geometry and result are those of that call
 * on the materialised block, bit for bit.
 *
 * Same contract as above (stream-ordered, no allocation, no host synchronisation,
 * graph-capturable, the timing hook goes to the aggregation's main kernel). Refused with
 * GNN_EINVAL before anything is launched: a negative size, rows, nnz or num_nodes >= 2^31,
 * row0 + rows > num_nodes, F > ldx or F > ldy, a kind other than 0, 1, 2, a workspace smaller than
 * gnn_spmm_graph_workspace_bytes(rows, nnz, F) or not 16-byte aligned, and for 16-bit X whatever
 * gnn_spmm_csr_h16_f32 refuses. That size is the row pointer, the weights and the aggregation's
 * gnn_spmm_workspace_bytes(rows, nnz, F, 0), each rounded up to 256 bytes — the last raised to a
 * bound that grows with rows and with nnz (the unit count of gnn_spmm_default_unit_nnz does not),
 * so the size is monotone in both and a workspace sized for a plan's largest block serves all. */
size_t gnn_spmm_graph_workspace_bytes(int64_t rows, int64_t nnz, int64_t F);
int gnn_spmm_graph_f32(const int64_t* indptr, const int32_t* indices, const int32_t* degree,
                       int64_t num_nodes, int64_t row0, int64_t rows, int64_t e0, int64_t nnz,
                       const void* X, int64_t ldx, int kind,
                       float* Y, int64_t ldy, int64_t F,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The same aggregation over a list of graph rows, with the columns relabelled to positions in a
 * node set — one layer of inference restricted to a query set's closure (gnn_extract.h:
 * gnn_closure_*):
 *     Y[i, 0:F] = w_i * sum over the entries e of graph row rows[i] of X[pos(indices[e]), 0:F],
 *     w_i = (float)(1.0 / (double)degree[rows[i]])
 * rows int32[M]: node ids in any order (repeats allowed); table: the membership table of the set
 * (gnn_closure_mark's, over num_nodes nodes), whose K members index X's K rows: pos(c) is c's
 * position in the ascending set. rowseg int32[M+1] (device) is the host-made exclusive scan of the
 * rows' degrees and nnz = rowseg[M] its total, as gnn_ladies_extract_f32 takes its offsets.
 *
 * One kernel writes the block-local CSR into the workspace: the row pointer from rowseg (clamped
 * to [0, nnz], ends pinned), col[e] = pos(indices[..]) (one 8-byte table load per entry, a row's
 * entries over a wave's lanes) and val[e] = w_i. The set is ascending and pos monotone, so columns
 * stay ascending per row. The sums are then gnn_spmm_csr_f32 / gnn_spmm_csr_h16_f32 on that
 * operand: kernel choice, geometry and result are that call's on the materialised block, bit for
 * bit. An entry whose column is not in the set (or any entry the inputs do not resolve: a position
 * not below K, a row id outside the graph, a scan longer than the graph's row) is stored as
 * column 0 with value 0 and ORs 1 into err_flag (device int32, optional): every stored column is
 * below K, so the aggregation stays inside X whatever the inputs hold.
 *
 * Contract and refusals as gnn_spmm_graph_f32 (M in place of rows), plus K >= 2^31, K > num_nodes
 * and a NULL table. The workspace, gnn_spmm_rows_workspace_bytes(M, nnz, F), is the row pointer,
 * the columns, the weights and gnn_spmm_graph_workspace_bytes's monotone bound for the
 * aggregation (its unit count cut at nnz / 4 + 1: a unit never holds fewer than 4 entries, so a
 * few-row block does not pay that bound's 2,048-unit floor), each rounded up to 256 bytes; monotone
 * in rows and nnz, never below gnn_spmm_workspace_bytes(M, nnz, F, 0). */
size_t gnn_spmm_rows_workspace_bytes(int64_t rows, int64_t nnz, int64_t F);
int gnn_spmm_rows_f32(const int64_t* indptr, const int32_t* indices, const int32_t* degree,
                      int64_t num_nodes, const int32_t* rows, int64_t M, const int32_t* rowseg,
                      int64_t nnz, const void* table, int64_t K,
                      const void* X, int64_t ldx, int kind,
                      float* Y, int64_t ldy, int64_t F,
                      void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream);

/* Optional timing hook: when set, the NEXT gnn_spmm_csr_f32 / gnn_spmm_csr_h16_f32 call on this thread launches its
 * main aggregation kernel with `start` / `stop` as the dispatch's own start and end timestamps
 * (hipExtLaunchKernel: hipEventElapsedTime(start, stop) = the kernel's duration, as rocprofv3
 * reports it), then clears the hook. Events are hipEvent_t (created with timing) as void*. */
void gnn_spmm_set_timing_events(void* start, void* stop);

/* ---------------------------------------------------------------------------------
 * Sampled-adjacency operand builder.
 *
 * Replaces: create_coo_tensor(fullrowptr, rowptr, colidx, normfact, nrows, ncols)
 *           spmm_cpp/spmm.cpp:44-50 -> to_coo_tensor / _create_coo_tensor_kernel
 *           spmm_cpp/cuda_spmm.cu:787-827 (called from sampler.py:135-139).
 * For row r and each entry i in [rowptr[r], rowptr[r+1]):
 *     val[i] = (float)((1.0 / (double)(fullrowptr[r+1] - fullrowptr[r])) * (double)normfact[col[i]])
 * (double arithmetic, single rounding to fp32, as cuda_spmm.cu:800).
 * colidx may be int16 (colidx_bytes = 2, sign-extended like the reference's int16
 * accessor), int32 (4) or int64 (8). Rows whose columns are not ascending are sorted
 * (key = column, payload = value), which is what the reference's .coalesce() does
 * (cuda_spmm.cu:825). A repeated column within a row (never made by scipy slicing or the
 * reference's samplers) is NOT merged here — merging changes nnz, which the host would have to
 * read back — but flagged: the workspace's second int64 word is nonzero after the call iff a row
 * repeats a column (checked after sorting), so a caller can coalesce lazily at a point that
 * synchronises anyway (gnn_amd.custom_sparse_ops: the first aggregation on the tensor).
 * Outputs: csr_col (int32, nnz), csr_val (fp32, nnz) and, if coo_indices != NULL, the
 * coalesced COO indices int64[2][nnz] (row-major: all rows then all columns).
 * `workspace` (device, 8-byte aligned, >= gnn_build_operand_workspace_bytes()) holds the
 * call's "unsorted row seen" and "repeated column seen" words, zeroed on `stream` by the call itself: the library keeps
 * no device state and allocates nothing, so the call is graph-capturable and concurrent
 * calls on different streams need different workspaces.
 * ------------------------------------------------------------------------------- */
size_t gnn_segsort_workspace_bytes(int64_t nseg);
size_t gnn_build_operand_workspace_bytes(void);
int gnn_build_operand_f32(const int32_t* fullrowptr, const int32_t* rowptr,
                          const void* colidx, int colidx_bytes,
                          const float* normfact, int64_t nrows, int64_t ncols, int64_t nnz,
                          int32_t* csr_col, float* csr_val, int64_t* coo_indices,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Same, for rows the caller guarantees column-ascending (e.g. gnn_ladies_sample output): no
 * unsorted-row check pass is launched (one launch instead of two). */
int gnn_build_operand_sorted_f32(const int32_t* fullrowptr, const int32_t* rowptr,
                                 const void* colidx, int colidx_bytes,
                                 const float* normfact, int64_t nrows, int64_t ncols, int64_t nnz,
                                 int32_t* csr_col, float* csr_val, int64_t* coo_indices, void* stream);

/* ---------------------------------------------------------------------------------
 * Format conversions (replace the per-call preprocessing of cuda_spmm.cu:620-667 and the
 * backward's A.transpose(0,1).coalesce() of custom_sparse_ops.py:34).
 * ------------------------------------------------------------------------------- */

/* Values of the TRANSPOSED operand (Aᵀ, K x M) when the caller already has A's CSC
 * structure (colptr int32[K+1], rows int32[nnz], rows ascending inside each column — e.g.
 * from gnn_ladies_layer_csc): val_t[i] = (float)((1.0/deg_full(rows[i])) * normfact[c]) for
 * the entries of column c, the forward's value of the same entry bit for bit. Then
 * (colptr, rows, val_t) is the canonical transpose (what gnn_csr_transpose builds on the GPU
 * and custom_sparse_ops.py:34 `A.transpose(0,1).coalesce()` computes). */
int gnn_build_operand_t_f32(const int32_t* fullrowptr, const int32_t* colptr, const int32_t* rows,
                            const float* normfact, int64_t nrows, int64_t ncols, int64_t nnz, float* val_t,
                            void* stream);

/* Coalesced COO (int64 row and column index arrays, rows ascending) -> CSR row pointer
 * (int32, M+1) and int32 column indices. `col32` may be NULL to skip the narrowing. */
int gnn_coo_to_csr(const int64_t* row, const int64_t* col, int64_t nnz, int64_t M,
                   int32_t* rowptr, int32_t* col32, void* stream);

/* CSR (M x K) -> CSR of the transpose (K x M), canonical: rows ascending inside every
 * output row, i.e. identical to A.t().coalesce(). Deterministic.
 * tr_rowptr: int32[K+1], tr_col: int32[nnz], tr_val: fp32[nnz].
 * `workspace` >= gnn_csr_transpose_workspace_bytes(M, K, nnz). */
size_t gnn_csr_transpose_workspace_bytes(int64_t M, int64_t K, int64_t nnz);
int gnn_csr_transpose(const int32_t* rowptr, const int32_t* col, const float* val,
                      int64_t M, int64_t K, int64_t nnz,
                      int32_t* tr_rowptr, int32_t* tr_col, float* tr_val,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Feature staging (replaces the masked gathers of main.py:129-134).
 * dst[dst_idx[i], 0:F] = src[src_idx[i], 0:F] for i in [0, n). A NULL src_idx / dst_idx
 * means the identity. Row strides in elements. Indices int64.
 * ------------------------------------------------------------------------------- */
int gnn_gather_rows_f32(const float* src, int64_t ld_src, const int64_t* src_idx,
                        float* dst, int64_t ld_dst, const int64_t* dst_idx,
                        int64_t n, int64_t F, void* stream);

/* Two sources in one launch (round 6): dst[pos0[i]] = src0[idx0[i]] for i < n0, then
 * dst[pos1[i]] = src1[idx1[i]] for i < n1 — the own feature-buffer rows and the batch's host
 * rows of one X0 (main.py:129-134). NULL idx / pos = identity. */
int gnn_gather_rows2_f32(const float* src0, int64_t ld0, const int64_t* idx0, const int64_t* pos0, int64_t n0,
                         const float* src1, int64_t ld1, const int64_t* idx1, const int64_t* pos1, int64_t n1,
                         float* dst, int64_t ld_dst, int64_t F, void* stream);

/* The same gathers from a 16-bit feature store, widening to fp32 on the way (the `.float()` of
 * main.py:132-134): dst[dst_idx[i], 0:F] = (float)src[src_idx[i], 0:F]. `kind` names the source
 * elements: GNN_FEAT_F16 (IEEE binary16) or GNN_FEAT_BF16; GNN_FEAT_F32 (0) is reserved for the
 * fp32 calls above and, like any other value, refused here with a status before anything is
 * launched. Both conversions are exact (finite values, zeros, subnormals, infinities; NaN stays
 * NaN). Source strides in 16-bit elements, any stride >= F and any 2-byte-aligned base; rows
 * whose stride and base are 16-byte aligned move by 16-byte loads. */
enum { GNN_FEAT_F32 = 0, GNN_FEAT_F16 = 1, GNN_FEAT_BF16 = 2 };
int gnn_gather_rows_h16_f32(const void* src, int64_t ld_src, int kind, const int64_t* src_idx,
                            float* dst, int64_t ld_dst, const int64_t* dst_idx,
                            int64_t n, int64_t F, void* stream);
/* Two 16-bit sources of the same kind in one launch (as gnn_gather_rows2_f32); rows too wide for
 * its one-pass kernel take gnn_gather_rows_h16_f32 per source. */
int gnn_gather_rows2_h16_f32(const void* src0, int64_t ld0, const int64_t* idx0, const int64_t* pos0, int64_t n0,
                             const void* src1, int64_t ld1, const int64_t* idx1, const int64_t* pos1, int64_t n1,
                             int kind, float* dst, int64_t ld_dst, int64_t F, void* stream);

/* Zero-copy variant for the non-buffered rows (replaces the pageable
 * feat_data[idx_cpu].to(device) of main.py:134): `host_src` is host memory registered with
 * gnn_host_register (pinned, device-mapped); the GPU reads the rows over PCIe, so no host
 * thread copies them. src_idx / dst_idx are device int64 arrays (NULL = identity). A small
 * persistent grid keeps the gather's CU footprint low beside the compute stream. */
int gnn_gather_rows_host_f32(const float* host_src, int64_t ld_src, const int64_t* src_idx,
                             float* dst, int64_t ld_dst, const int64_t* dst_idx,
                             int64_t n, int64_t F, void* stream);

/* X0 by node id over a placed feature store: dst[i, 0:F] = (float) row(nodes[i])[0:F], where the
 * row's source is looked up on the device, in this rank's placement map — the device draws'
 * (gnn_extract.h: gnn_nbr_*, gnn_lw_*) input nodes exist only there, so no host mask, slot list
 * or compaction can be made for them (main.py:129-134 assembles X0 from the same three sources by
 * host masks).
 *
 * place int32[num_nodes] (device): GNN_PLACE_HOST (-1) = the row is row `node` of the host table;
 * otherwise src << GNN_PLACE_SHIFT | slot: row `slot` of source `src` — the reference's
 * device_id_of_nodes and idx_of_nodes_on_device (preprocess.py:343-386) in one word. srcs (device,
 * nsrc <= GNN_PLACE_MAX_SRC entries, uploaded once): per source its base, row stride `ld` in its
 * elements and row count; source 0 is the rank's own buffer, the others mapped peer buffers
 * (gnn_ipc_open). `kind` (GNN_FEAT_*) names the elements of every source and of the host table;
 * 16-bit rows are widened exactly. host_table is host memory registered with gnn_host_register
 * (NULL: none), any stride ld_host >= F and any element-aligned base; nodes int32[n] (device).
 *
 * One launch: the first workgroups (at most 32) walk the positions for host-placed nodes — a
 * contiguous range per wave, 64 map values at a time, the host ones balloted and read over PCIe two
 * rows at a time — while the others take one device row per wave; the load width is chosen per
 * source from its base and stride, within what dst allows, so a narrow host table does not
 * narrow the buffer rows; a row's columns past its last whole vector move one per lane, so F need
 * not be a multiple of the width (602-column rows move by 16-byte loads). counts (device int64[nsrc + 1], may be NULL) is ADDED to: the rows each
 * source served, the host last (one relaxed add per walker wave; integer adds, so deterministic).
 *
 * A row that cannot be served is stored as zeros and ORs 1 into *flag (device int32): a node
 * outside [0, num_nodes), a source index >= nsrc, a slot >= its source's rows, a source with a NULL
 * base or ld < F, a host-placed node with a NULL host_table. Nothing outside a source is read.
 * Stream-ordered, no allocation, no host read, graph-capturable. Refused with GNN_EINVAL before
 * anything is launched: an unknown kind, nsrc outside [1, 16], a negative size, num_nodes, n or F
 * >= 2^31, F > ld_dst, F > ld_host (with a host table) and, for n > 0 and F > 0, a NULL place, srcs,
 * nodes, dst or flag or a misaligned host_table / dst. */
#define GNN_PLACE_HOST (-1)
#define GNN_PLACE_SHIFT 27
#define GNN_PLACE_MAX_SRC 16
typedef struct gnn_place_src {
  const void* base;
  int64_t ld;
  int64_t rows;
} gnn_place_src;
int gnn_gather_placed_f32(const int32_t* place, int64_t num_nodes,
                          const gnn_place_src* srcs, int nsrc,
                          const void* host_table, int64_t ld_host,
                          int kind,
                          const int32_t* nodes, int64_t n,
                          float* dst, int64_t ld_dst, int64_t F,
                          int64_t* counts, int32_t* flag, void* stream);

/* Pin + map a host range for device access (hipHostRegister, mapped) / undo it. */
int gnn_host_register(void* host, size_t bytes);
int gnn_host_unregister(void* host);

/* Peer feature buffers read directly over xGMI (replaces the per-peer
 * gpu_buffers[i][idx].to(device) P2P copies of main.py:129-133 without any per-step collective):
 * each rank exports its buffer ONCE — an IPC handle of the allocation holding `ptr` and the byte
 * offset of `ptr` in that allocation — the peers open it ONCE (peer access to `peer_device`
 * enabled when it is another GPU), and gnn_gather_rows_f32 then reads a batch's peer rows
 * straight from the mapped pointer into X0. The buffer must stay allocated and unchanged while
 * peers hold it mapped; gnn_ipc_close undoes gnn_ipc_open. */
#define GNN_IPC_HANDLE_BYTES 64
int gnn_ipc_export(const void* ptr, void* handle_out, int64_t* offset_out);
int gnn_ipc_open(const void* handle, int64_t offset, int peer_device, void** ptr_out);
int gnn_ipc_close(void* ptr, int64_t offset);

/* A stream whose kernels run only on `cus` of the device's CUs, spread evenly over its CU
 * numbering (hipExtStreamCreateWithCUMask; a blocking stream) — experiments with the X0 staging
 * stream (GNN_STAGE_CUS). gnn_stream_destroy releases it. */
int gnn_stream_create_cu_masked(int32_t device, int32_t cus, int32_t priority, void** stream_out);
int gnn_stream_destroy(void* stream);

/* One stream-ordered host-to-device copy (hipMemcpyAsync): the upload of a native loader's
 * batch blob (gnn_sampler.h) — every per-batch array of main.py:115-134 in one transfer. */
int gnn_memcpy_h2d_async(void* dst, const void* src, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GNN_SPMM_H */
