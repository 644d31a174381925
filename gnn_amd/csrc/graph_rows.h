// graph_rows.h — device helpers the samplers over the resident graph share (neighbor.hip,
// layerwise.hip): a graph row's span with its bounds checked, and a node's position in a
// membership table (closure.hip's word).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

namespace gnn {

// The graph row of node r: its first entry and its degree. False (and d = 0) for a node outside
// the graph or a row pointer that would put a read outside [0, E).
__device__ __forceinline__ bool row_span(const int64_t* __restrict__ indptr, int N, int64_t E, int r, int64_t& b,
                                         int& d) {
  b = 0;
  d = 0;
  if ((unsigned)r >= (unsigned)N) return false;
  const int64_t b0 = indptr[r], e0 = indptr[r + 1];
  if (b0 < 0 || e0 < b0 || e0 > E || e0 - b0 >= (int64_t)INT_MAX) return false;
  b = b0;
  d = (int)(e0 - b0);
  return true;
}

// The position of node c in the ascending set of a membership table over N nodes (one uint2 per 32
// ids: x = the bits, y = the members below the word); -1 for a non-member or an id outside [0, N).
__device__ __forceinline__ int table_pos(const uint2* __restrict__ tab, int N, int c) {
  if ((unsigned)c >= (unsigned)N) return -1;
  const uint2 wd = tab[c >> 5];
  const unsigned sh = (unsigned)c & 31u;
  if (!((wd.x >> sh) & 1u)) return -1;
  return (int)(wd.y + (unsigned)__builtin_popcount(wd.x & ((1u << sh) - 1u)));
}

}  // namespace gnn
