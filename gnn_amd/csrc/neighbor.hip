// neighbor.hip — node-wise neighbour sampling over the resident graph (include/gnn_extract.h:
// gnn_nbr_*): every output row keeps k = min(deg, fanout) of its graph row's entries, a uniform
// k-subset without replacement, each with the weight (float)(1.0 / (double)k) — lap's 1/deg times
// deg/k, an unbiased estimate of lap[r, :], and the row itself whenever deg <= fanout.
//
// The draw is a pure integer function of (seed, layer, node id, deg, fanout): the same row comes
// out wherever it sits in the batch and whichever device draws it (gnn_amd/neighbor.py restates it
// in numpy, the tests' oracle).
//   key = mix32((mix32(lo32(seed) ^ 0x9e3779b9) ^ hi32(seed)) + layer * 0x85EBCA6B)   (host)
//   rk  = mix32(node ^ key)
//   deg <= fanout: every entry. Otherwise Floyd's algorithm, for s = 0 .. k-1:
//     j = deg - k + s,  u = mix32(rk ^ mix32(s + 0x632BE5AB)),  t = (uint64(u) * (j + 1)) >> 32,
//     insert j if t is in the set already, else t.
//   The kept entries are those positions of the row, in ascending order.
//
// Launches, all on the caller's stream, stream order the only synchronisation between workgroups:
//   gnn_nbr_rowptr   nb_chunk_scan (k per row, scanned inside chunks of 8,192 rows: closure.hip's
//                    cl_chunk_scan shape), scan_exclusive over the chunk sums, nb_chunk_add (also
//                    rowptr[M] and *total)
//   gnn_nbr_draw     nb_draw: a wave per row, grid-stride. The wave holds the growing set one
//                    element per lane. Lane s computes step s's candidate t on its own, before the
//                    loop (the hashes do not depend on the set), so step s is a broadcast of lane
//                    s's t, one ballot (is t in the set?) and a select into lane s: exactly k <= 64
//                    steps, no data-dependent exit. Ascending order is a rank count (the lanes
//                    holding a smaller position, k broadcasts); lane i then loads its one entry of
//                    the row and stores id and weight at rowptr[row] + rank. Only k entries of a
//                    row are read, whatever its degree.
//   gnn_nbr_relabel  a thread per entry: its id's position in a gnn_closure_mark table, as int32
// Memory safety does not depend on the inputs' contents: a row id outside [0, num_nodes), a row
// pointer outside [0, num_entries] or running backwards, and an output offset outside [0, cap]
// give the row k = 0 / skip it; a column id outside the graph is stored as id -1 with weight 0
// (gnn_closure_mark skips it, gnn_nbr_relabel makes it column 0). Each of these ORs 1 into err_flag.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "common.h"
#include "gnn_extract.h"
#include "graph_rows.h"

namespace {

using gnn::align_up;
using gnn::ceil_div;
using gnn::row_span;

using Word = uint2;  // extract.hip's membership word
constexpr int NB_ITEMS = 8;
constexpr int NB_CHUNK = 1024 * NB_ITEMS;  // rows per scan workgroup
constexpr int NB_DRAW_WAVES = 4;           // waves per drawing workgroup
constexpr int NB_DRAW_GRID = 4096;         // at most this many drawing workgroups
constexpr int NB_MAX_FANOUT = 64;          // one set element per lane

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {  // sage.hip's "lowbias32"
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// rowptr of workgroup j's rows = the exclusive scan of their k within the chunk; csum[j] = the
// chunk's entries
__global__ __launch_bounds__(1024) void nb_chunk_scan_kernel(const int64_t* __restrict__ indptr, int N, int64_t E,
                                                             const int32_t* __restrict__ rows, int M, int f,
                                                             int32_t* __restrict__ rowptr, int32_t* __restrict__ csum,
                                                             int32_t* __restrict__ err) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * NB_CHUNK + (int64_t)tid * NB_ITEMS;
  int v[NB_ITEMS];
  int tsum = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < NB_ITEMS; ++k) {
    v[k] = 0;
    if (base + k < M) {
      int64_t b;
      int d;
      bad |= !row_span(indptr, N, E, rows[base + k], b, d);
      v[k] = d < f ? d : f;
    }
    tsum += v[k];
  }
  if (bad && err) atomicOr(err, 1);
  int x = tsum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  if (wave == 0) {
    int w = lane < 16 ? wsum[lane] : 0;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const int y = __shfl_up(w, d);
      if (lane >= d) w += y;
    }
    if (lane < 16) wsum[lane] = w;
  }
  __syncthreads();
  int excl = (wave ? wsum[wave - 1] : 0) + x - tsum;
#pragma unroll
  for (int k = 0; k < NB_ITEMS; ++k) {
    if (base + k < M) rowptr[base + k] = excl;
    excl += v[k];
  }
  if (tid == 0) csum[blockIdx.x] = wsum[15];
}

// rowptr += the chunk's start; thread M writes rowptr[M] and *total
__global__ __launch_bounds__(256) void nb_chunk_add_kernel(int32_t* __restrict__ rowptr, int M,
                                                           const int32_t* __restrict__ coff, int nchunks,
                                                           int64_t* __restrict__ total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < M) {
    rowptr[i] += coff[i / NB_CHUNK];
  } else if (i == M) {
    rowptr[M] = coff[nchunks];
    *total = (int64_t)coff[nchunks];
  }
}

__global__ __launch_bounds__(64 * NB_DRAW_WAVES) void nb_draw_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int N, int64_t E,
    const int32_t* __restrict__ rows, int M, int f, uint32_t key, const int32_t* __restrict__ rowptr,
    int32_t* __restrict__ ids, float* __restrict__ val, int64_t cap, int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * NB_DRAW_WAVES + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * NB_DRAW_WAVES;
  for (int64_t i = wave; i < M; i += nwaves) {  // everything but `mine`, `rank` and `c` is wave-uniform
    const int r = rows[i];
    int64_t b;
    int d;
    bool bad = !row_span(indptr, N, E, r, b, d);
    const int k = d < f ? d : f;
    const int64_t o = rowptr[i];
    if (k > 0 && (o < 0 || o + k > cap)) {  // not this call's row pointer: nothing is written
      if (lane == 0 && err) atomicOr(err, 1);
      continue;
    }
    int mine = lane;  // d <= f: every entry, already in order
    int rank = lane;
    if (d > f) {
      const uint32_t rk = mix32((uint32_t)r ^ key);
      // lane s's candidate of step s (j + 1 = d - k + s + 1 <= d < 2^31)
      const uint32_t u = mix32(rk ^ mix32((uint32_t)lane + 0x632BE5ABu));
      const int tl = (int)(((uint64_t)u * (uint64_t)((uint32_t)(d - k) + (uint32_t)lane + 1u)) >> 32);
      mine = -1;
      for (int s = 0; s < k; ++s) {
        const int t = __shfl(tl, s);
        const unsigned long long hit = __ballot(lane < s && mine == t);
        if (lane == s) mine = hit ? d - k + s : t;
      }
      rank = 0;
      for (int s = 0; s < k; ++s) rank += __shfl(mine, s) < mine ? 1 : 0;
    }
    if (lane < k) {
      int c = indices[b + mine];  // mine < d: inside the row
      float w = (float)(1.0 / (double)k);
      if ((unsigned)c >= (unsigned)N) {
        c = -1;
        w = 0.0f;
        bad = true;
      }
      ids[o + rank] = c;
      val[o + rank] = w;
    }
    if (__ballot(bad) && lane == 0 && err) atomicOr(err, 1);
  }
}

__global__ __launch_bounds__(256) void nb_relabel_kernel(const Word* __restrict__ tab, int N,
                                                         const int32_t* __restrict__ ids, int64_t n,
                                                         int32_t* __restrict__ col, float* __restrict__ val,
                                                         int32_t* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = ids[i];
  int p = -1;
  if ((unsigned)c < (unsigned)N) {
    const Word wd = tab[c >> 5];
    const unsigned sh = (unsigned)c & 31u;
    if ((wd.x >> sh) & 1u) p = (int)(wd.y + (unsigned)__builtin_popcount(wd.x & ((1u << sh) - 1u)));
  }
  col[i] = p < 0 ? 0 : p;
  if (p < 0) {
    if (val) val[i] = 0.0f;
    if (err) atomicOr(err, 1);
  }
}

inline size_t chunk_bytes(int64_t M) {
  return align_up(((size_t)ceil_div(M, (int64_t)NB_CHUNK) + 1) * sizeof(int32_t), 256);
}

}  // namespace

extern "C" {

size_t gnn_nbr_workspace_bytes(int64_t M) {
  return 2 * chunk_bytes(M > 0 ? M : 0);  // the chunk sums and their scan
}

int gnn_nbr_rowptr(const int64_t* indptr, int64_t num_nodes, int64_t num_entries, const int32_t* rows, int64_t M,
                   int32_t fanout, int32_t* rowptr, int64_t* total, void* workspace, size_t workspace_bytes,
                   int32_t* err_flag, void* stream) {
  GNN_REQUIRE(num_nodes >= 0 && num_entries >= 0 && M >= 0, "gnn_nbr_rowptr: negative size (num_nodes, num_entries or M)");
  GNN_REQUIRE(num_nodes < INT_MAX && M < INT_MAX, "gnn_nbr_rowptr: num_nodes and M must be < 2^31");
  GNN_REQUIRE(fanout >= 1 && fanout <= NB_MAX_FANOUT, "gnn_nbr_rowptr: fanout %d outside [1, %d]", (int)fanout,
              NB_MAX_FANOUT);
  GNN_REQUIRE(M * (int64_t)fanout < INT_MAX, "gnn_nbr_rowptr: M * fanout must be < 2^31");
  GNN_REQUIRE(rowptr && total, "gnn_nbr_rowptr: NULL rowptr/total");
  GNN_REQUIRE(M == 0 || (indptr && rows), "gnn_nbr_rowptr: NULL indptr/rows");
  const size_t need = gnn_nbr_workspace_bytes(M);
  GNN_REQUIRE(workspace && workspace_bytes >= need, "gnn_nbr_rowptr: workspace too small (%zu < %zu)",
              workspace ? workspace_bytes : (size_t)0, need);
  GNN_REQUIRE((uintptr_t)workspace % 16 == 0, "gnn_nbr_rowptr: workspace not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nch = (int)ceil_div(M, (int64_t)NB_CHUNK);
  int32_t* csum = (int32_t*)workspace;
  int32_t* coff = (int32_t*)((char*)workspace + chunk_bytes(M));
  if (nch > 0) {
    nb_chunk_scan_kernel<<<dim3((unsigned)nch), dim3(1024), 0, st>>>(indptr, (int)num_nodes, num_entries, rows, (int)M,
                                                                     (int)fanout, rowptr, csum, err_flag);
    GNN_LAUNCHED("nb_chunk_scan_kernel");
  }
  int rc = gnn::launch_scan_exclusive(csum, nch, coff, st);
  if (rc) return rc;
  nb_chunk_add_kernel<<<dim3((unsigned)ceil_div(M + 1, 256)), dim3(256), 0, st>>>(rowptr, (int)M, coff, nch, total);
  GNN_LAUNCHED("nb_chunk_add_kernel");
  return 0;
}

int gnn_nbr_draw(const int64_t* indptr, const int32_t* indices, int64_t num_nodes, int64_t num_entries,
                 const int32_t* rows, int64_t M, int32_t fanout, uint64_t seed, int32_t layer, const int32_t* rowptr,
                 int32_t* ids, float* val, int64_t cap, int32_t* err_flag, void* stream) {
  GNN_REQUIRE(num_nodes >= 0 && num_entries >= 0 && M >= 0 && cap >= 0,
              "gnn_nbr_draw: negative size (num_nodes, num_entries, M or cap)");
  GNN_REQUIRE(num_nodes < INT_MAX && M < INT_MAX, "gnn_nbr_draw: num_nodes and M must be < 2^31");
  GNN_REQUIRE(fanout >= 1 && fanout <= NB_MAX_FANOUT, "gnn_nbr_draw: fanout %d outside [1, %d]", (int)fanout,
              NB_MAX_FANOUT);
  GNN_REQUIRE(M * (int64_t)fanout < INT_MAX, "gnn_nbr_draw: M * fanout must be < 2^31");
  if (M == 0) return 0;
  GNN_REQUIRE(indptr && rows && rowptr, "gnn_nbr_draw: NULL indptr/rows/rowptr");
  GNN_REQUIRE(num_entries == 0 || indices, "gnn_nbr_draw: NULL indices");
  GNN_REQUIRE(cap == 0 || (ids && val), "gnn_nbr_draw: NULL ids/val");
  const uint32_t key =
      mix32((mix32((uint32_t)seed ^ 0x9e3779b9u) ^ (uint32_t)(seed >> 32)) + (uint32_t)layer * 0x85EBCA6Bu);
  const int64_t g = ceil_div(M, (int64_t)NB_DRAW_WAVES);
  nb_draw_kernel<<<dim3((unsigned)(g < NB_DRAW_GRID ? g : NB_DRAW_GRID)), dim3(64 * NB_DRAW_WAVES), 0,
                   (hipStream_t)stream>>>(indptr, indices, (int)num_nodes, num_entries, rows, (int)M, (int)fanout, key,
                                          rowptr, ids, val, cap, err_flag);
  GNN_LAUNCHED("nb_draw_kernel");
  return 0;
}

int gnn_nbr_relabel(const void* table, int64_t num_nodes, const int32_t* ids, int64_t n, int32_t* col, float* val,
                    int32_t* err_flag, void* stream) {
  GNN_REQUIRE(num_nodes >= 0 && n >= 0, "gnn_nbr_relabel: negative size (num_nodes or n)");
  GNN_REQUIRE(num_nodes < INT_MAX && n < INT_MAX, "gnn_nbr_relabel: num_nodes and n must be < 2^31");
  GNN_REQUIRE(table != nullptr, "gnn_nbr_relabel: NULL table");
  GNN_REQUIRE((uintptr_t)table % 8 == 0, "gnn_nbr_relabel: table not 8-byte aligned");
  if (n == 0) return 0;
  GNN_REQUIRE(ids && col, "gnn_nbr_relabel: NULL ids/col");
  nb_relabel_kernel<<<dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream>>>(
      (const Word*)table, (int)num_nodes, ids, n, col, val, err_flag);
  GNN_LAUNCHED("nb_relabel_kernel");
  return 0;
}

}  // extern "C"
