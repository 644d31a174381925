/* gnn_extract.h — C ABI of the GPU-side LADIES layer extraction (libgnn_spmm.so, gfx950).
 *
 * Replaces, for every sampled layer whose rows are unique and ascending (all layers below the
 * top one: their rows are the np.unique output of the layer above), the host half of
 *   reference sampler.py:114   U = lap_matrix[previous_nodes, :]
 *   reference sampler.py:133   adj = U[:, after_nodes]
 *   reference sampler.py:135-139  rowptr / colidx / normfact -> create_coo_tensor
 * and the device half, create_coo_tensor (spmm_cpp/spmm.cpp:44-50 -> cuda_spmm.cu:787-827),
 * in one stream-ordered call that reads the graph's CSR resident in device memory. The host
 * sampler keeps the draw (np.random.choice over the column counts of U) and hands over the rows
 * (previous_nodes), the columns (after_nodes), normfact, and — from the same column counts —
 * the exact nnz and the CSC column pointer of adj.
 *
 * Conventions as gnn_spmm.h: device pointers, a hipStream_t as void*, no host syncs, no
 * allocation (graph-capturable), 0 on success / negative or hipError_t code with the message in
 * gnn_last_error().
 */
#ifndef GNN_EXTRACT_H
#define GNN_EXTRACT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The operand of one sampled layer and, optionally, its transpose.
 *
 * Graph (device): the lap matrix as canonical CSR (indptr int64[num_nodes+1], indices int32,
 * columns ascending per row, no duplicates); indptr_t / indices_t: the same for lap^T (may alias
 * indptr / indices when the structure is symmetric). deg(v) = indptr[v+1] - indptr[v]; degree
 * int32[num_nodes] holds it (required with the transpose: its values' row degrees).
 * rows  int32[M]: U's rows (node ids) in order; cols int32[K]: after_nodes, strictly ascending;
 * normfact fp32[K]; nnz = number of entries of U[:, cols] (the sum of U's column counts over cols).
 * rowseg int32[M+1] = U's row pointer (exclusive scan of deg(rows[i])); colseg int32[K+1] = the
 * exclusive scan of lapᵀ's row lengths of cols (transpose only) — both host-known (the draw).
 * workspace: gnn_ladies_extract_workspace_bytes(num_nodes, M, K, transpose, rowseg_total,
 * colseg_total) bytes (8 bytes per graph entry scanned plus tables; no state is kept between
 * calls: concurrent calls on different streams need different workspaces).
 * Outputs: rowptr int32[M+1], col int32[nnz] (positions into cols, ascending per row),
 * val fp32[nnz] = (float)((1.0 / deg(rows[i])) * (double)normfact[col]) — identical to
 * gnn_build_operand_f32 on the host-extracted pieces with fullrowptr = rowseg.
 * Transpose (colptr_t != NULL; rows must then be unique and ascending): rows_t int32[nnz] /
 * val_t fp32[nnz] receive the canonical CSR of adj^T (rows ascending in each column) whose row
 * pointer is colptr_t, the host's CSC column pointer (its column counts; not read here) — what
 * gnn_csr_transpose / A.t().coalesce() would produce.
 * rowseg_total = rowseg[M] and colseg_total = colseg[K] (transpose only; ignored otherwise): the
 * graph entries scanned per direction, host-known like the offsets (they size the launch).
 * Work is balanced over entries, not rows (power-law rows): each direction's concatenated graph
 * rows are cut into equal contiguous ranges, one per wave, and every entry is read ONCE (the
 * kept entries of a range go to a gapped buffer, then to their place after a scan of the
 * per-range counts); membership of a node in cols / rows is a bitmap + per-word rank table.
 * err_flag (device int32, optional): OR-ed with 1 / 2 if the kept entries of A / A^T do not add up
 * to nnz (or a segment total differs from the device offsets). The outputs then stay safe to
 * read: writes stay below nnz, entries past the kept ones are zero-filled (column / row 0, value
 * 0) and rowptr is clamped to nnz. */
size_t gnn_ladies_extract_workspace_bytes(int64_t num_nodes, int64_t M, int64_t K, int32_t transpose,
                                          int64_t rowseg_total, int64_t colseg_total);
int gnn_ladies_extract_f32(const int64_t* indptr, const int32_t* indices, const int32_t* degree, int64_t num_nodes,
                           const int64_t* indptr_t, const int32_t* indices_t, const int32_t* rows, int64_t M, const int32_t* cols, int64_t K,
                           const float* normfact, int64_t nnz, const int32_t* rowseg, const int32_t* colseg,
                           const int32_t* colptr_t, int64_t rowseg_total, int64_t colseg_total, int32_t* rowptr,
                           int32_t* col, float* val, int32_t* rows_t, float* val_t, void* workspace,
                           size_t workspace_bytes, int32_t* err_flag, void* stream);

/* U's column counts for the LADIES draw on the GPU (reference sampler.py:116-122,
 * pi = norm(U, ord=0, axis=0)), for a host sampler thread (gnn_sampler.h: gnn_colcount_api).
 * A context belongs to ONE host thread: its own stream, a device count array over the graph's
 * nodes, pinned result buffers. Unlike the rest of this library these calls synchronise with
 * their own stream (the host draw needs the result) and gnn_colcount_create allocates.
 * create: graph = the lap matrix's canonical CSR in device memory (as gnn_ladies_extract_f32;
 *   no stored zeros), device = the HIP device it lives on.
 * add: count the entries of lap rows rows[0..n) (host node ids; repeats count again) into the
 *   context's counts, then return the non-zero columns: *bits = bitmap (host, ceil(N/64) words,
 *   bit c%64 of word c/64), *counts = their counts in ascending column order (host, *nlive
 *   entries). Both stay valid until the next call on the context.
 * reset: zero the counts (stream-ordered before the next add).
 * The counts are summed without global atomics (a bucket partition + LDS histograms) unless
 * GNN_CC_HIST=atomic is set when the context is created; same counts either way. GNN_CC_CUS=n:
 * the context's stream on n of the device's CUs (own hardware queue; default: a plain stream).
 * Note: hipExtStreamCreateWithCUMask makes a BLOCKING stream (the default is non-blocking), so
 * with GNN_CC_CUS set the counter's work also orders against legacy null-stream work; the bench's
 * producers issue none (torch and the library use explicit streams), off by default.
 * A call's entry total is carried in int64; a call of 2^31 or more entries (beyond the int32
 * partition offsets) runs the atomic form instead. */
int gnn_colcount_create(int32_t device, int64_t num_nodes, const int64_t* indptr, const int32_t* indices, void** ctx);
/* The stream of the contexts created after this call (process-wide): cus = 0 a plain stream
 * (default), cus > 0 a stream over that many CUs (>= the device's: all of them) — a CU-masked
 * stream gets a hardware queue of its own instead of sharing one with the training step's streams
 * (GPU_MAX_HW_QUEUES is 4). GNN_CC_CUS, when set, overrides. Returns 0, or -22 for cus < 0. */
int gnn_colcount_set_cus(int32_t cus);
int gnn_colcount_add(void* ctx, const int64_t* rows, int64_t n, int64_t* nlive, const uint64_t** bits,
                     const int32_t** counts);
int gnn_colcount_reset(void* ctx);
void gnn_colcount_destroy(void* ctx);

/* Node sets on the device, for inference restricted to a query set's k-hop closure (closure.hip).
 * A set S over num_nodes nodes is its membership table, the word of the extraction above: one
 * 8-byte word (uint32 x, uint32 y) per 32 node ids — x = the ids of [32 w, 32 w + 32) as bits,
 * y = the number of members below 32 w — and one trailing word (x = 0, y = |S|). The position of
 * node c in ascending S is y + popcount(x & ((1 << c % 32) - 1)) of word c / 32.
 * gnn_closure_table_bytes(num_nodes): the table's size; gnn_closure_workspace_bytes(num_nodes):
 * gnn_closure_mark's scratch (the scan's chunk sums). Both are rounded up to 256 bytes.
 *
 * mark: table = the membership table of seeds int32[n] (any order, repeats allowed) and, with
 *   expand != 0, of every column of lap[seeds, :] as well (indices[indptr[s] .. indptr[s+1]) for
 *   each seed s; the graph as gnn_ladies_extract_f32 takes it). *count (device int64) = |S|.
 *   A wave per seed, its row's entries over the lanes; bits are OR-ed atomically (relaxed), the
 *   ranks are a chunked scan: five launches in stream order, no workgroup waits for another.
 *   Seeds and columns outside [0, num_nodes) are skipped. n = 0 gives the empty table, count 0.
 * list: out[0 .. min(|S|, cap)) = the members in ascending order; nothing is written at or past cap.
 * rank: pos[i] (int64, the index type of gnn_gather_rows_f32) = the position of ids[i] in S; an id
 *   outside S gets position 0 and ORs 1 into err_flag (device int32, optional).
 *
 * Conventions as above: device pointers, stream-ordered, no allocation, no host synchronisation.
 * Refused with GNN_EINVAL before anything is launched: a negative size, num_nodes or n >= 2^31, a
 * NULL or misaligned table, a NULL count / seeds / ids / pos / out where one is read or written, a
 * workspace that is NULL, too small or not 16-byte aligned. */
size_t gnn_closure_table_bytes(int64_t num_nodes);
size_t gnn_closure_workspace_bytes(int64_t num_nodes);
int gnn_closure_mark(const int64_t* indptr, const int32_t* indices, int64_t num_nodes, const int32_t* seeds, int64_t n,
                     int32_t expand, void* table, int64_t* count, void* workspace, size_t workspace_bytes,
                     void* stream);
int gnn_closure_list(const void* table, int64_t num_nodes, int32_t* out, int64_t cap, void* stream);
int gnn_closure_rank(const void* table, int64_t num_nodes, const int32_t* ids, int64_t n, int64_t* pos,
                     int32_t* err_flag, void* stream);

/* Node-wise neighbour sampling over the resident graph (neighbor.hip): the layer operand of a
 * GraphSAGE-style draw with a fanout per layer. The graph as above (lap's canonical CSR, no stored
 * values: every entry of row r weighs 1/deg(r)); num_entries = the length of indices. Output row i
 * (node rows[i]; any order, repeats allowed) keeps k_i = min(deg(rows[i]), fanout) entries of its
 * graph row, a uniform k_i-subset without replacement, each with the weight
 * (float)(1.0 / (double)k_i) — an unbiased estimate of lap[rows[i], :], and the row itself when
 * deg <= fanout. 1 <= fanout <= 64.
 *
 * The draw is a pure integer function of (seed, layer, node id, deg, fanout), so a row's entries
 * do not depend on its place in the batch or on the device. With mix32 the "lowbias32" hash of
 * the dropout masks (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16),
 * in 32-bit arithmetic:
 *   key = mix32((mix32(lo32(seed) ^ 0x9e3779b9) ^ hi32(seed)) + layer * 0x85EBCA6B)
 *   rk  = mix32(node ^ key)
 *   deg <= fanout: every entry. Otherwise (Floyd), for s = 0 .. k-1: j = deg - k + s,
 *   u = mix32(rk ^ mix32(s + 0x632BE5AB)), t = (uint64(u) * (j + 1)) >> 32; insert j if t is in
 *   the set already, else t. The kept entries are those positions of the row, ascending.
 *
 * rowptr: rowptr int32[M+1] = the exclusive scan of k_i, *total (device int64) = rowptr[M];
 *   workspace = gnn_nbr_workspace_bytes(M) bytes (the scan's chunk sums), 16-byte aligned.
 * draw: ids int32[cap] / val fp32[cap] receive, at rowptr[i] .. rowptr[i+1], row i's kept global
 *   column ids in ascending order and their weights; rowptr as gnn_nbr_rowptr made it with the same
 *   rows and fanout; cap = the capacity of ids / val (M * fanout always suffices). Only the kept
 *   entries of a row are read.
 * relabel: col[e] = the position of ids[e] in the ascending set of a gnn_closure_mark table, as
 *   int32 (a CsrOperand's column type), e < n. An id outside the set becomes column 0, with
 *   val[e] = 0 when val is given.
 * A layer's input set is gnn_closure_mark(seeds = rows ++ ids, expand = 0) + gnn_closure_list.
 *
 * Memory safety does not depend on the contents of the device arrays: a row id outside
 * [0, num_nodes), or a row pointer outside [0, num_entries] or running backwards, gives the row
 * k = 0; a row whose output range leaves [0, cap] is skipped; a column id outside the graph is
 * stored as id -1 with weight 0 (gnn_closure_mark skips it, relabel makes it column 0). Each
 * case ORs 1 into err_flag (device int32, optional).
 *
 * Conventions as above: device pointers, stream-ordered, no allocation, no host synchronisation.
 * Refused with GNN_EINVAL before anything is launched: a negative size, num_nodes, M or n >= 2^31,
 * M * fanout >= 2^31, fanout outside [1, 64], a NULL pointer where one is read or written, a
 * misaligned table, a workspace that is NULL, too small or not 16-byte aligned. */
size_t gnn_nbr_workspace_bytes(int64_t M);
int gnn_nbr_rowptr(const int64_t* indptr, int64_t num_nodes, int64_t num_entries, const int32_t* rows, int64_t M,
                   int32_t fanout, int32_t* rowptr, int64_t* total, void* workspace, size_t workspace_bytes,
                   int32_t* err_flag, void* stream);
int gnn_nbr_draw(const int64_t* indptr, const int32_t* indices, int64_t num_nodes, int64_t num_entries,
                 const int32_t* rows, int64_t M, int32_t fanout, uint64_t seed, int32_t layer, const int32_t* rowptr,
                 int32_t* ids, float* val, int64_t cap, int32_t* err_flag, void* stream);
int gnn_nbr_relabel(const void* table, int64_t num_nodes, const int32_t* ids, int64_t n, int32_t* col, float* val,
                    int32_t* err_flag, void* stream);

/* The LADIES layer draw on the device: a hashed race over the resident graph (layerwise.hip).
 *
 * The reference (sampler.py:113-139) takes U = lap[rows, :] (rows: the layer's output nodes, in
 * order, repeats kept), pi = U's entry count per column, p = pi / sum(pi), s_num = min(number of
 * live columns, samp_num), and draws np.random.choice(N, s_num, p = p, replace = False):
 * successive sampling without replacement, proportional to integer weights. The same law comes from
 * a race: give every entry of U an independent uniform value and every column the maximum over its
 * entries; the overall maximum is equally likely to be any entry, so column j leads with
 * probability pi_j / sum(pi), and removing that column leaves the same situation among the rest.
 * The s_num columns with the largest maxima are distributed exactly as np.random.choice's set.
 *
 * The draw, in 64-bit unsigned arithmetic mod 2^64 (a pure integer function of the seed):
 *   mix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *             z ^= z >> 31                                   (the splitmix64 finaliser)
 *   K = mix64(seed + (layer + 1) * 0x9E3779B97F4A7C15), layer = the model's layer index (0 = bottom)
 *   the entry of U in row position i (its index in rows, not the node id: a repeated row counts
 *   again, as the reference's U does) and column node id c:  h(i, c) = mix64((c << 32 | i) + K)
 *   key[c] = max_i h(i, c), count[c] = the number of entries; a column is live iff count[c] > 0.
 *   mix64 is a bijection and (c, i) is unique per entry, so all entry values, hence all column
 *   keys, are distinct: no tie rule exists or is needed.
 *   s_num = min(nlive, samp_num); selected = the s_num live columns with the largest keys;
 *   after = unique(selected ++ rows);
 *   normfact[k] = 1.0f / (float)clip((double)s_num * ((double)count[after[k]] / (double)sum(count)),
 *                                    1e-10, 1.0)
 *   (sampler.py:137: the clipped value is cast to float32 before the reciprocal, a float32 division;
 *   the ratio counts as 0 when nothing was counted). A row node that is nobody's column has count 0,
 *   hence normfact 1 / float32(1e-10) and an empty column. adj = lap[rows, :][:, after] with
 *   gnn_ladies_extract_f32's values.
 *
 * A layer on the device, everything on one stream up to one read of (K, totals, flag):
 *   gnn_closure_mark(seeds = rows, expand = 1) -> the live table: the columns of U and (the mark sets
 *     its seeds too) the rows themselves, ntab members;  gnn_closure_list -> tab_ids
 *   gnn_lw_race -> count, key, sum(count);  gnn_lw_select -> s_num, tau, ids
 *   gnn_closure_mark(seeds = rows ++ ids, expand = 0) -> the table of after, K;  gnn_closure_list -> after
 *   gnn_lw_finish -> normfact and gnn_ladies_extract_f32's offsets and totals.
 *
 * race: count int32[cap] / key uint64[cap], indexed by the column's position in the live table (its
 *   rank lookup: no array over num_nodes), are zero-filled and then filled; *total (device int64) =
 *   sum(count). cap >= ntab; min(num_nodes, M + sum of deg(rows)) suffices. A member that is only a
 *   row keeps count 0 and key 0. A wave per row, the row's entries over the lanes; one 32-bit add
 *   and one 64-bit max per entry.
 * select: over the positions j < *ntab (device int64, clamped to cap) with count[j] > 0, the nlive
 *   live columns: *s_num (device int64) = min(nlive, samp_num), *tau (device uint64) = the s_num-th
 *   largest of their keys (0 when s_num = 0), ids[j] = (count[j] > 0 and key[j] >= tau) ?
 *   tab_ids[j] : -1 for j < ntab and -1 for ntab <= j < cap (gnn_closure_mark skips -1: no
 *   compaction). An exact radix select on the full 64 bits, eight passes of LDS histograms, its
 *   state kept in the workspace (gnn_lw_select_workspace_bytes()); exactly s_num entries pass,
 *   because keys are distinct. Nothing at or past ntab is read.
 * finish: for after int32[*K] (*K device int64, clamped to kcap; the list of the second table):
 *   normfact fp32[K] (count looked up through the live table, 0 for a non-member),
 *   colptr_t int32[K+1] = the exclusive scan of count[after] (closing entry: the operand's nnz),
 *   rowseg int32[M+1] = the scan of deg(rows), colseg int32[K+1] = the scan of lap^T's row lengths
 *   of after, totals int64[3] (device) = nnz, colseg[K], sum of deg(after) (the next layer's
 *   rowseg[M]). A sum of 2^31 or more ORs 1 into err_flag; its offsets are then all zero and its
 *   total reads 2^31 - 1, so the outputs stay safe to read. workspace:
 *   gnn_lw_finish_workspace_bytes(M, kcap).
 *
 * The locality-skewed draw (gnn_lw_race_skew, gnn_lw_finish_skew; the reference's sampler.py:119-121
 * with preprocess.get_skewed_sampled_nodes: pi of a column that is cheap to fetch is multiplied by
 * scale_factor before the draw, and normfact comes from the skewed p, so the estimator stays
 * LADIES's). Inputs: scale, an integer in [1, 64], and the layer's favoured set F, a subset of
 * [0, num_nodes), as a bit table favoured uint32[ceil(num_nodes / 32)] (device, 4-byte aligned):
 * node c is bit c & 31 of word c >> 5.
 *   s(c) = scale if c is in F, else 1. The entry of U in row position i and column c has s(c)
 *   replicas; replica r (0 <= r < s(c)) has the value
 *     h_r(i, c) = mix64((c << 32 | r << 26 | i) + K),   K as above; h_0 = h.
 *   This needs i < 2^26: a skewed race over M >= 2^26 rows is refused. c < 2^31, r < 2^6 and
 *   i < 2^26 occupy disjoint bit fields, so (c, r, i) is unique per replica, and mix64 being a
 *   bijection all replica values, hence all column keys, are distinct: still no tie rule.
 *   key[c] = max over i and r of h_r(i, c): the maximum of w[c] = count[c] * s(c) independent
 *   uniform values, so the race is successive sampling without replacement proportional to w,
 *   the law of np.random.choice(p = pi * scale / sum, replace = False).
 *   count[c] stays the raw entry count (colptr_t, the operand's nnz and gnn_ladies_extract_f32's
 *   cross-check read it as such); *total = sum of w[c] (int64), w formed in 64 bits;
 *   normfact[k] = 1.0f / (float)clip((double)s_num * ((double)w[after[k]] / (double)total),
 *                                    1e-10, 1.0)
 *   (sampler.py:137 on the scaled pi; for integer scales every intermediate is exact in fp64).
 *   With F empty, favoured == NULL or scale == 1 this is the plain draw bit for bit, and
 *   gnn_lw_race / gnn_lw_finish are the skewed entry points called with (NULL, 1). Only integer
 *   scales: a fractional weight has no exact integer race. gnn_lw_select is the same for both:
 *   its liveness rule is count > 0 and keys are distinct.
 *   race_skew: per entry, after the live table's lookup, one 4-byte read of the favoured word; the
 *   replicas' maximum is taken in registers, so an entry still issues one 32-bit add and one
 *   64-bit max; a wave adds the sum of s(c) to *total. finish_skew: the same scans, normfact's
 *   weight alone becomes count * s(after[k]).
 *
 * Memory safety does not depend on the contents of the device arrays: a row id outside
 * [0, num_nodes), a row pointer outside [0, num_entries] or running backwards, a column that is not
 * in the live table or sits at a position >= cap contribute nothing; *ntab and *K are clamped to
 * cap and kcap. Each case ORs 1 into err_flag (device int32, optional). The skewed draw adds no
 * case: the favoured word's index derives from a column that has passed the live table's lookup,
 * so 0 <= c < num_nodes and the word lies inside the table whatever the arrays hold.
 *
 * Conventions as above: device pointers, stream-ordered, no allocation, no host synchronisation.
 * Refused with GNN_EINVAL before anything is launched: a negative size, a size >= 2^31,
 * samp_num < 1, a negative layer, a NULL pointer where one is read or written, a misaligned table
 * or 8-byte word, a workspace that is NULL, too small or not 16-byte aligned; of the skewed entry
 * points also scale outside [1, 64], a favoured table that is not 4-byte aligned, and scale > 1
 * with a table and M >= 2^26. */
int gnn_lw_race(const int64_t* indptr, const int32_t* indices, int64_t num_nodes, int64_t num_entries,
                const int32_t* rows, int64_t M, const void* live_table, uint64_t seed, int32_t layer, int32_t* count,
                uint64_t* key, int64_t cap, int64_t* total, int32_t* err_flag, void* stream);
size_t gnn_lw_select_workspace_bytes(void);
int gnn_lw_select(const uint64_t* key, const int32_t* count, const int64_t* ntab, int64_t cap, int64_t samp_num,
                  const int32_t* tab_ids, int32_t* ids, int64_t* s_num, uint64_t* tau, void* workspace,
                  size_t workspace_bytes, void* stream);
size_t gnn_lw_finish_workspace_bytes(int64_t M, int64_t kcap);
int gnn_lw_finish(const int64_t* indptr, int64_t num_entries, const int64_t* indptr_t, int64_t num_entries_t,
                  int64_t num_nodes, const int32_t* rows, int64_t M, const int32_t* after, const int64_t* K,
                  int64_t kcap, const void* live_table, const int32_t* count, int64_t cap, const int64_t* total,
                  const int64_t* s_num, float* normfact, int32_t* colptr_t, int32_t* rowseg, int32_t* colseg,
                  int64_t* totals, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream);
int gnn_lw_race_skew(const int64_t* indptr, const int32_t* indices, int64_t num_nodes, int64_t num_entries,
                     const int32_t* rows, int64_t M, const void* live_table, uint64_t seed, int32_t layer,
                     int32_t* count, uint64_t* key, int64_t cap, int64_t* total, int32_t* err_flag, void* stream,
                     const uint32_t* favoured, int32_t scale);
int gnn_lw_finish_skew(const int64_t* indptr, int64_t num_entries, const int64_t* indptr_t, int64_t num_entries_t,
                       int64_t num_nodes, const int32_t* rows, int64_t M, const int32_t* after, const int64_t* K,
                       int64_t kcap, const void* live_table, const int32_t* count, int64_t cap, const int64_t* total,
                       const int64_t* s_num, float* normfact, int32_t* colptr_t, int32_t* rowseg, int32_t* colseg,
                       int64_t* totals, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream,
                       const uint32_t* favoured, int32_t scale);

/* The subgraph sampler's batch on the device (the reference's sampler.py:7-88): ONE draw over the
 * batch rows, then every layer below the drawn one aggregates over the same induced square operand.
 *
 * The law. orders[l] in {0, 1}, bottom-up; t = the topmost layer with orders[t] = 1; rows = the batch
 * nodes (M of them, any order, repeats allowed).
 *   The draw is the race above over U = lap[rows, :] with layer = t: the same K, h, h_r, count, key
 *   and select, samp_num = the reference's samp_num_list[0] (sampler.py:28), and optionally one
 *   favoured set with an integer scale in [1, 64] (the reference's own set is the nodes placed on the
 *   drawing device, sampler.py:23-25).
 *   after = unique(selected ++ rows), K of them; normfact as gnn_lw_finish_skew writes it
 *   (sampler.py:40).
 *   Layer t: adj = lap[rows, :][:, after] with gnn_ladies_extract_f32's values and sampled_nodes = the
 *   positions of rows in after — for the same (rows, seed, samp_num) bit for bit the top layer of the
 *   layer-wise draw.
 *   Every layer l < t with orders[l] = 1: the square operand S = lap[after, :][:, after] (K x K),
 *   S's value at (i, col) = (float)((1.0 / deg(after[i])) * (double)normfact[col]) with the same
 *   normfact array (sampler.py:62), sampled_nodes = 0 .. K-1. S is built once per batch.
 *   An order-0 layer has no operand. The input nodes are after.
 *
 * S by gnn_ladies_extract_f32(rows = cols = after) needs, beyond gnn_lw_finish's colseg (the scan of
 * lap^T's row lengths of after), S's nnz, its row segments and the row pointer of its transpose:
 * count: for k < *K (device int64, clamped to kcap) colcnt[k] = the number of entries of lap^T's row
 *   after[k] (indptr_t / indices_t, which may alias lap's when the structure is symmetric) that are
 *   members of table, the gnn_closure_mark table of after: the entry count of S's column k. Taken
 *   over lap^T the count needs no atomic and does not depend on the schedule: a wave per k,
 *   grid-stride, the row's entries over the lanes, the wave sums the popcounts of its ballots and
 *   lane 0 stores. Nothing is written at or past min(*K, kcap).
 * finish: colptr_t int32[K+1] = the exclusive scan of colcnt (closing entry: S's nnz), rowseg
 *   int32[K+1] = the exclusive scan of deg(after[k]) over lap, totals int64[2] (device) = S's nnz and
 *   rowseg[K]. gnn_lw_finish's chunked scans and its overflow rule: a sum of 2^31 or more ORs 1 into
 *   err_flag, its offsets are then all zero and its total reads 2^31 - 1. *K above kcap is clamped
 *   and flagged. workspace: gnn_sg_finish_workspace_bytes(kcap), 16-byte aligned.
 *
 * Memory safety does not depend on the contents of the device arrays: a member of after outside
 * [0, num_nodes), or a row pointer outside [0, num_entries] or running backwards, counts 0 and ORs 1
 * into err_flag (device int32, optional); an entry of lap^T outside [0, num_nodes) is no member.
 *
 * Conventions as above: device pointers, stream-ordered, no allocation, no host synchronisation.
 * Refused with GNN_EINVAL before anything is launched: a negative size, a size >= 2^31, a NULL
 * pointer where one is read or written, a misaligned table or 8-byte word, a workspace that is
 * NULL, too small or not 16-byte aligned. */
int gnn_sg_count(const int64_t* indptr_t, const int32_t* indices_t, int64_t num_nodes, int64_t num_entries_t,
                 const int32_t* after, const int64_t* K, int64_t kcap, const void* table, int32_t* colcnt,
                 int32_t* err_flag, void* stream);
size_t gnn_sg_finish_workspace_bytes(int64_t kcap);
int gnn_sg_finish(const int64_t* indptr, int64_t num_entries, int64_t num_nodes, const int32_t* after,
                  const int64_t* K, int64_t kcap, const int32_t* colcnt, int32_t* colptr_t, int32_t* rowseg,
                  int64_t* totals, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GNN_EXTRACT_H */
