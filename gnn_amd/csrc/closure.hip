// closure.hip — node sets on the GPU for inference restricted to a query set's k-hop closure
// (include/gnn_extract.h: gnn_closure_*).
//
// Exact inference at a set of nodes needs, per layer, the set of nodes whose activations the
// layer above reads: S' = S ∪ cols(lap[S, :]). The graph is resident (sampler.DeviceGraph), so a
// hop is grown where it lies: the members become bits of extract.hip's membership table (one
// 8-byte word per 32 node ids: x = the bits, y = the members below the word), which is at once
// the set (gnn_closure_list), the map node id -> position in the ascending set (gnn_closure_rank)
// and the column relabelling of the layer's aggregation (gnn_spmm_rows_f32).
//
// gnn_closure_mark, all on the caller's stream, stream order the only synchronisation between
// workgroups (no look-back, no spinning, no cooperative launch):
//   memset          the table's bits and ranks to zero
//   cl_mark         a wave per seed (grid-stride over the seeds): lane 0 sets the seed's bit; with
//                   expand the lanes stride the seed's row, 64 entries a step, so a row of 10^5
//                   entries is ~1,600 steps of one wave and never one lane's loop. Bits are set
//                   with relaxed agent-scope atomic ORs (idempotent: any order gives the same
//                   table). A row's columns ascend, so the lanes of a step that fall into one word
//                   are neighbours: they OR their bits together over the lanes first and the run's
//                   first lane issues one atomic for the run (at most 32-way contention on one
//                   address becomes one access). The runs are also cut at lane 32, which bounds a
//                   run at 32 lanes whatever the input holds (a row with repeated columns too).
//   cl_chunk_scan   workgroup j scans the popcounts of its 8,192 words into their y and leaves
//                   the chunk's sum in csum[j] (colcount.hip's cc_chunk_scan shape)
//   scan_exclusive  the chunk sums (one workgroup, any count)
//   cl_chunk_add    y += the chunk's start; the trailing word and *count receive the total
// Ids outside [0, num_nodes) — seeds or graph entries — are skipped: the table never gets a bit
// past its last word.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "common.h"
#include "gnn_extract.h"

namespace {

using gnn::align_up;
using gnn::ceil_div;

using Word = uint2;  // extract.hip's membership word
constexpr int WORD_NODES = 32;
constexpr int CL_ITEMS = 8;
constexpr int CL_CHUNK = 1024 * CL_ITEMS;  // words per scan workgroup (262,144 node ids)
constexpr int CL_MARK_WAVES = 4;           // waves per marking workgroup
constexpr int CL_MARK_GRID = 4096;         // at most this many marking workgroups

inline int64_t table_words(int64_t num_nodes) { return ceil_div(num_nodes, (int64_t)WORD_NODES); }

__device__ __forceinline__ void set_bits(Word* tab, int w, unsigned bits) {
  __hip_atomic_fetch_or(&tab[w].x, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(64 * CL_MARK_WAVES) void cl_mark_kernel(const int64_t* __restrict__ indptr,
                                                                     const int32_t* __restrict__ indices, int N,
                                                                     const int32_t* __restrict__ seeds, int n, int expand,
                                                                     Word* __restrict__ tab) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * CL_MARK_WAVES + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * CL_MARK_WAVES;
  for (int64_t r = wave; r < n; r += nwaves) {
    const int s = seeds[r];
    if ((unsigned)s >= (unsigned)N) continue;  // wave-uniform
    if (lane == 0) set_bits(tab, s >> 5, 1u << (s & 31));
    if (!expand) continue;
    const int64_t b = indptr[s], e = indptr[s + 1];
    for (int64_t k0 = b; k0 < e; k0 += 64) {  // wave-uniform trip count: the shuffles see all lanes
      const int64_t k = k0 + lane;
      const int c = k < e ? indices[k] : -1;
      const bool valid = (unsigned)c < (unsigned)N;
      const int w = valid ? (c >> 5) : -1 - lane;  // an invalid lane is a run of its own
      unsigned bits = valid ? 1u << (c & 31) : 0u;
      const int prev = __shfl_up(w, 1);
      const bool head = (lane & 31) == 0 || prev != w;
#pragma unroll
      for (int d = 1; d < 32; d <<= 1) {  // OR over the run: same word, same half of the wave
        const unsigned ob = __shfl_down(bits, d);
        const int ow = __shfl_down(w, d);
        if (((lane + d) >> 5) == (lane >> 5) && ow == w) bits |= ob;
      }
      if (head && valid) set_bits(tab, w, bits);
    }
  }
}

// y of workgroup j's words = the exclusive scan of their popcounts within the chunk; csum[j] = the
// chunk's members
__global__ __launch_bounds__(1024) void cl_chunk_scan_kernel(Word* __restrict__ tab, int words,
                                                             int32_t* __restrict__ csum) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * CL_CHUNK + (int64_t)tid * CL_ITEMS;
  int v[CL_ITEMS];
  int tsum = 0;
#pragma unroll
  for (int k = 0; k < CL_ITEMS; ++k) {
    v[k] = base + k < words ? __builtin_popcount(tab[base + k].x) : 0;
    tsum += v[k];
  }
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
  for (int k = 0; k < CL_ITEMS; ++k) {
    if (base + k < words) tab[base + k].y = (unsigned)excl;
    excl += v[k];
  }
  if (tid == 0) csum[blockIdx.x] = wsum[15];
}

// y += the chunk's start; thread `words` writes the trailing word (no bits, y = |S|) and *count
__global__ __launch_bounds__(256) void cl_chunk_add_kernel(Word* __restrict__ tab, int words,
                                                           const int32_t* __restrict__ coff, int nchunks,
                                                           int64_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < words) {
    tab[i].y += (unsigned)coff[i / CL_CHUNK];
  } else if (i == words) {
    tab[words] = make_uint2(0u, (unsigned)coff[nchunks]);
    *count = (int64_t)coff[nchunks];
  }
}

// a thread per node id: the members written at their positions (below cap)
__global__ __launch_bounds__(256) void cl_list_kernel(const Word* __restrict__ tab, int N, int32_t* __restrict__ out,
                                                      int64_t cap) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const Word wd = tab[c >> 5];
  const unsigned sh = (unsigned)c & 31u;
  if (!((wd.x >> sh) & 1u)) return;
  const int64_t p = (int64_t)wd.y + __builtin_popcount(wd.x & ((1u << sh) - 1u));
  if (p < cap) out[p] = (int32_t)c;
}

__global__ __launch_bounds__(256) void cl_rank_kernel(const Word* __restrict__ tab, int N,
                                                      const int32_t* __restrict__ ids, int64_t n,
                                                      int64_t* __restrict__ pos, int32_t* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = ids[i];
  int64_t p = -1;
  if ((unsigned)c < (unsigned)N) {
    const Word wd = tab[c >> 5];
    const unsigned sh = (unsigned)c & 31u;
    if ((wd.x >> sh) & 1u) p = (int64_t)wd.y + __builtin_popcount(wd.x & ((1u << sh) - 1u));
  }
  pos[i] = p < 0 ? 0 : p;
  if (p < 0 && err) atomicOr(err, 1);
}

}  // namespace

extern "C" {

size_t gnn_closure_table_bytes(int64_t num_nodes) {
  const int64_t n = num_nodes > 0 ? num_nodes : 0;
  return align_up(((size_t)table_words(n) + 1) * sizeof(Word), 256);
}

size_t gnn_closure_workspace_bytes(int64_t num_nodes) {
  const int64_t n = num_nodes > 0 ? num_nodes : 0;
  const size_t nch = (size_t)ceil_div(table_words(n), (int64_t)CL_CHUNK);
  return 2 * align_up((nch + 1) * sizeof(int32_t), 256);  // the chunk sums and their scan
}

int gnn_closure_mark(const int64_t* indptr, const int32_t* indices, int64_t num_nodes, const int32_t* seeds, int64_t n,
                     int32_t expand, void* table, int64_t* count, void* workspace, size_t workspace_bytes,
                     void* stream) {
  GNN_REQUIRE(num_nodes >= 0 && n >= 0, "gnn_closure_mark: negative size (num_nodes or n)");
  GNN_REQUIRE(num_nodes < INT_MAX && n < INT_MAX, "gnn_closure_mark: num_nodes and n must be < 2^31");
  GNN_REQUIRE(table != nullptr, "gnn_closure_mark: NULL table");
  GNN_REQUIRE((uintptr_t)table % 8 == 0, "gnn_closure_mark: table not 8-byte aligned");
  GNN_REQUIRE(count != nullptr, "gnn_closure_mark: NULL count");
  const size_t need = gnn_closure_workspace_bytes(num_nodes);
  GNN_REQUIRE(workspace && workspace_bytes >= need, "gnn_closure_mark: workspace too small (%zu < %zu)",
              workspace ? workspace_bytes : (size_t)0, need);
  GNN_REQUIRE((uintptr_t)workspace % 16 == 0, "gnn_closure_mark: workspace not 16-byte aligned");
  GNN_REQUIRE(n == 0 || seeds, "gnn_closure_mark: NULL seeds");
  GNN_REQUIRE(n == 0 || !expand || (indptr && indices), "gnn_closure_mark: NULL indptr/indices with expand");
  hipStream_t st = (hipStream_t)stream;
  const int words = (int)table_words(num_nodes);
  const int nch = (int)ceil_div(words, CL_CHUNK);
  Word* tab = (Word*)table;
  int32_t* csum = (int32_t*)workspace;
  int32_t* coff = (int32_t*)((char*)workspace + align_up(((size_t)nch + 1) * sizeof(int32_t), 256));
  GNN_HIP(hipMemsetAsync(tab, 0, ((size_t)words + 1) * sizeof(Word), st), "hipMemsetAsync");
  if (n > 0 && words > 0) {
    const int64_t g = ceil_div(n, (int64_t)CL_MARK_WAVES);
    cl_mark_kernel<<<dim3((unsigned)(g < CL_MARK_GRID ? g : CL_MARK_GRID)), dim3(64 * CL_MARK_WAVES), 0, st>>>(
        indptr, indices, (int)num_nodes, seeds, (int)n, expand ? 1 : 0, tab);
    GNN_LAUNCHED("cl_mark_kernel");
  }
  if (nch > 0) {
    cl_chunk_scan_kernel<<<dim3((unsigned)nch), dim3(1024), 0, st>>>(tab, words, csum);
    GNN_LAUNCHED("cl_chunk_scan_kernel");
  }
  int rc = gnn::launch_scan_exclusive(csum, nch, coff, st);
  if (rc) return rc;
  cl_chunk_add_kernel<<<dim3((unsigned)ceil_div((int64_t)words + 1, 256)), dim3(256), 0, st>>>(tab, words, coff, nch,
                                                                                              count);
  GNN_LAUNCHED("cl_chunk_add_kernel");
  return 0;
}

int gnn_closure_list(const void* table, int64_t num_nodes, int32_t* out, int64_t cap, void* stream) {
  GNN_REQUIRE(num_nodes >= 0 && cap >= 0, "gnn_closure_list: negative size (num_nodes or cap)");
  GNN_REQUIRE(num_nodes < INT_MAX, "gnn_closure_list: num_nodes must be < 2^31");
  GNN_REQUIRE(table != nullptr, "gnn_closure_list: NULL table");
  GNN_REQUIRE((uintptr_t)table % 8 == 0, "gnn_closure_list: table not 8-byte aligned");
  if (num_nodes == 0 || cap == 0) return 0;
  GNN_REQUIRE(out != nullptr, "gnn_closure_list: NULL out");
  cl_list_kernel<<<dim3((unsigned)ceil_div(num_nodes, 256)), dim3(256), 0, (hipStream_t)stream>>>(
      (const Word*)table, (int)num_nodes, out, cap);
  GNN_LAUNCHED("cl_list_kernel");
  return 0;
}

int gnn_closure_rank(const void* table, int64_t num_nodes, const int32_t* ids, int64_t n, int64_t* pos,
                     int32_t* err_flag, void* stream) {
  GNN_REQUIRE(num_nodes >= 0 && n >= 0, "gnn_closure_rank: negative size (num_nodes or n)");
  GNN_REQUIRE(num_nodes < INT_MAX && n < INT_MAX, "gnn_closure_rank: num_nodes and n must be < 2^31");
  GNN_REQUIRE(table != nullptr, "gnn_closure_rank: NULL table");
  GNN_REQUIRE((uintptr_t)table % 8 == 0, "gnn_closure_rank: table not 8-byte aligned");
  if (n == 0) return 0;
  GNN_REQUIRE(ids && pos, "gnn_closure_rank: NULL ids/pos");
  cl_rank_kernel<<<dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream>>>(
      (const Word*)table, (int)num_nodes, ids, n, pos, err_flag);
  GNN_LAUNCHED("cl_rank_kernel");
  return 0;
}

}  // extern "C"
