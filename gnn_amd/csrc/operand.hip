// operand.hip — building the aggregation's CSR operands and converting between sparse formats:
// the operand builders (forward, pre-sorted and transposed values), COO -> CSR, the two CSR
// transposes (tiled counting sort for K <= 32 k, atomic slot claim + segmented sort beyond), the
// one-workgroup exclusive scan other translation units launch too, and the segmented sorters.
// Kernels and the gnn_build_operand* / gnn_coo_to_csr / gnn_csr_transpose* C ABI.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "gnn_spmm.h"
#include "common.h"
#include "spmm_device.h"

namespace {

using gnn::align_up;
using gnn::ceil_div;

// ---------------------------------------------------------------------------------
// Operand builder: value = (float)((1.0 / full_degree(row)) * (double)normfact[col]),
// the formula of cuda_spmm.cu:800 evaluated in double. A flat nnz-balanced pass builds
// every entry; rows found out of column order (never from a scipy-sliced sub-graph, but a
// caller may pass them) are redone by a row-per-wave pass that also sorts them.
// ---------------------------------------------------------------------------------
// Bitonic sort helpers, "all comparators ascending" form: positions >= L act as +inf.
constexpr int SEG_WAVE_LDS = 512;
constexpr int SEG_BLOCK_LDS = 16384;

__device__ __forceinline__ void cmpx_reg(int& k, float& v, int lane, int mask) {
  const int pk = __shfl_xor(k, mask);
  const float pv = __shfl_xor(v, mask);
  const bool lower = lane < (lane ^ mask);
  const bool take = lower ? (pk < k) : (pk > k);
  if (take) {
    k = pk;
    v = pv;
  }
}

// Pair p of a bitonic step -> element positions (i < j).
__device__ __forceinline__ void bitonic_pair(int p, int size, int d, bool flip, int& i, int& j) {
  if (flip) {
    const int half = size >> 1;
    i = (p / half) * size + (p % half);
    j = i ^ (size - 1);
  } else {
    i = (p / d) * (2 * d) + (p % d);
    j = i + d;
  }
}

// One row by one wave: values, a sortedness check and, for an unsorted row, the sort that
// restores the coalesced (column-ascending) order the reference gets from .coalesce():
// in registers (<= 64 entries), in the wave's LDS (<= 512) or in place in global memory.
template <typename CT>
__device__ void build_operand_row(const int* __restrict__ fullrowptr, const int* __restrict__ rowptr,
                                  const CT* __restrict__ colidx, const float* __restrict__ normfact, int r,
                                  int* __restrict__ out_col, float* __restrict__ out_val, int* sk, float* sv,
                                  int lane, unsigned long long* __restrict__ dflag, unsigned long long gen) {
  const int b = rowptr[r];
  const int e = rowptr[r + 1];
  if (b == e) return;
  const double inv = 1.0 / (double)(fullrowptr[r + 1] - fullrowptr[r]);
  bool bad = false;
  for (int i = b + lane; i < e; i += 64) {
    const int c = (int)colidx[i];
    if (i + 1 < e) bad |= c > (int)colidx[i + 1];
    out_col[i] = c;
    out_val[i] = (float)(inv * (double)normfact[c]);
  }
  if (__ballot(bad) == 0ull) return;
  const int L = e - b;
  if (L <= 64) {
    // this wave wrote the row above; re-read it (same lanes' own stores) and sort in registers
    int k = INT_MAX;
    float v = 0.0f;
    if (lane < L) {
      k = (int)colidx[b + lane];
      v = (float)(inv * (double)normfact[k]);
    }
    for (int size = 2; size <= 64; size <<= 1) {
      cmpx_reg(k, v, lane, size - 1);
      for (int d = size >> 2; d >= 1; d >>= 1) cmpx_reg(k, v, lane, d);
    }
    if (lane < L) {
      out_col[b + lane] = k;
      out_val[b + lane] = v;
    }
    // a repeated column, adjacent once sorted: flagged for the caller's lazy coalesce
    const int kn = __shfl_down(k, 1);
    if (dflag && __ballot(lane + 1 < L && k == kn) != 0ull && lane == 0) atomicMax(dflag, gen);
    return;
  }
  // Longer unsorted rows (never produced by scipy slicing, kept for generality): bitonic
  // sort of (column, value) by this wave, in its LDS region (<= 512) or in place in global
  // memory (the lanes' own stores are made visible to the wave by a workgroup fence).
  int n = 1;
  while (n < L) n <<= 1;
  if (L <= SEG_WAVE_LDS) {
    for (int i = lane; i < n; i += 64) {
      const int c = (i < L) ? (int)colidx[b + i] : INT_MAX;
      sk[i] = c;
      sv[i] = (i < L) ? (float)(inv * (double)normfact[c]) : 0.0f;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
  for (int size = 2; size <= n; size <<= 1) {
    for (int d = size >> 1; d >= 1; d >>= 1) {
      const bool flip = (d == (size >> 1));
      for (int p = lane; p < (n >> 1); p += 64) {
        int i, j;
        bitonic_pair(p, size, d, flip, i, j);
        if (L <= SEG_WAVE_LDS) {
          const int ki = sk[i], kj = sk[j];
          if (kj < ki) {
            const float vi = sv[i], vj = sv[j];
            sk[i] = kj;
            sk[j] = ki;
            sv[i] = vj;
            sv[j] = vi;
          }
        } else if (j < L) {
          const int ki = out_col[b + i], kj = out_col[b + j];
          if (kj < ki) {
            const float vi = out_val[b + i], vj = out_val[b + j];
            out_col[b + i] = kj;
            out_col[b + j] = ki;
            out_val[b + i] = vj;
            out_val[b + j] = vi;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
  }
  bool dup = false;
  if (L <= SEG_WAVE_LDS) {
    for (int i = lane; i < L; i += 64) {
      out_col[b + i] = sk[i];
      out_val[b + i] = sv[i];
      dup |= i + 1 < L && sk[i] == sk[i + 1];
    }
  } else {
    for (int i = lane; i + 1 < L; i += 64) dup |= out_col[b + i] == out_col[b + i + 1];
  }
  if (dflag && __ballot(dup) != 0ull && lane == 0) atomicMax(dflag, gen);
}

// Row-per-wave build with the sort fallback; grid-stride over rows. With `flag`, a no-op
// unless the flat builder of the same call (generation `gen`) saw an unsorted row.
template <typename CT>
__global__ __launch_bounds__(256) void build_operand_kernel(
    const int* __restrict__ fullrowptr, const int* __restrict__ rowptr,
    const CT* __restrict__ colidx, const float* __restrict__ normfact, int nrows,
    int* __restrict__ out_col, float* __restrict__ out_val,
    unsigned long long* __restrict__ flag, unsigned long long gen) {
  __shared__ int sk[4][SEG_WAVE_LDS];
  __shared__ float sv[4][SEG_WAVE_LDS];
  if (flag && flag[0] < gen) return;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  for (int r = blockIdx.x * 4 + w; r < nrows; r += gridDim.x * 4)
    build_operand_row<CT>(fullrowptr, rowptr, colidx, normfact, r, out_col, out_val, sk[w], sv[w], lane,
                          flag ? flag + 1 : nullptr, gen);
}

// nonzeros per wave in the flat operand builders (a multiple of 64)
#ifndef GNN_BUILD_CHUNK
#define GNN_BUILD_CHUNK 64
#endif
constexpr int BUILD_CHUNK = GNN_BUILD_CHUNK;

// Flat build: a wave per 256 consecutive nonzeros (nnz-balanced, ~4 loads in flight per
// lane), each lane finding its row by a short binary search between the chunk's first and
// last rows. Writes col/val for every entry and raises `flag` to `gen` if any row is out of
// order (then the row-per-wave kernel above re-does those rows with their sort).
template <typename CT>
__global__ __launch_bounds__(256) void build_operand_flat_kernel(
    const int* __restrict__ fullrowptr, const int* __restrict__ rowptr,
    const CT* __restrict__ colidx, const float* __restrict__ normfact, int nrows, int nnz,
    int* __restrict__ out_col, float* __restrict__ out_val,
    unsigned long long* __restrict__ flag, unsigned long long gen) {
  const int lane = threadIdx.x & 63;
  const int cs = (blockIdx.x * 4 + (threadIdx.x >> 6)) * BUILD_CHUNK;
  if (cs >= nnz) return;
  const int ce = min(cs + BUILD_CHUNK, nnz);
  const int rf = wave_first_true(0, nrows, lane, [&](int r) { return rowptr[r + 1] > cs; });
  // The ends of rows rf, rf+1, ... one per lane; entry i is in row rf + #{ends <= i}. When
  // fewer than 64 row ends fall inside the chunk that count is a uniform loop over them
  // (no per-entry search of rowptr in global memory).
  const int e = (rf + 1 + lane <= nrows) ? rowptr[rf + 1 + lane] : INT_MAX;
  const int nin = __popcll(__ballot(e < ce));
  int rl = rf;
  if (nin == 64) rl = wave_first_true(rf, nrows, lane, [&](int r) { return rowptr[r + 1] >= ce; });
  bool bad = false, dup = false;
#pragma unroll
  for (int t = 0; t < BUILD_CHUNK / 64; ++t) {
    const int i = cs + t * 64 + lane;
    int k = 0;
    if (nin < 64) {
      for (int j = 0; j < nin; ++j) k += (i >= __builtin_amdgcn_readlane(e, j)) ? 1 : 0;
    }
    const int rend = __shfl(e, k < 64 ? k : 63);
    if (i < ce) {
      int lo = rf + k, end = rend;
      if (nin == 64) {  // the largest r with rowptr[r] <= i is the row holding i
        int hi = rl;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (rowptr[mid] <= i) lo = mid; else hi = mid - 1;
        }
        end = rowptr[lo + 1];
      }
      const int c = (int)colidx[i];
      if (i + 1 < end) {
        const int cn = (int)colidx[i + 1];
        bad |= c > cn;
        dup |= c == cn;
      }
      const double inv = 1.0 / (double)(fullrowptr[lo + 1] - fullrowptr[lo]);
      out_col[i] = c;
      out_val[i] = (float)(inv * (double)normfact[c]);
    }
  }
  if (flag && __ballot(bad) != 0ull && lane == 0) atomicMax(flag, gen);
  // word 1: a repeated column in an already ascending row (unsorted rows: checked after their sort)
  if (flag && __ballot(dup) != 0ull && lane == 0) atomicMax(flag + 1, gen);
}

// Values of the transposed operand from its CSR structure (the CSC of A): entry i of
// transposed row c (a column of A) is A's entry (rows[i], c), value
// (float)((1.0 / full_degree(rows[i])) * (double)normfact[c]) — bit-identical to the
// forward operand's value of that entry, so (colptr, rows, val) IS the canonical transpose.
__global__ __launch_bounds__(256) void build_operand_t_kernel(
    const int* __restrict__ fullrowptr, const int* __restrict__ colptr, const int* __restrict__ rows,
    const float* __restrict__ normfact, int ncols, int nnz, float* __restrict__ out_val) {
  const int lane = threadIdx.x & 63;
  const int cs = (blockIdx.x * 4 + (threadIdx.x >> 6)) * BUILD_CHUNK;
  if (cs >= nnz) return;
  const int ce = min(cs + BUILD_CHUNK, nnz);
  const int cf = wave_first_true(0, ncols, lane, [&](int c) { return colptr[c + 1] > cs; });
  // column ends one per lane, as in build_operand_flat_kernel
  const int e = (cf + 1 + lane <= ncols) ? colptr[cf + 1 + lane] : INT_MAX;
  const int nin = __popcll(__ballot(e < ce));
  int cl = cf;
  if (nin == 64) cl = wave_first_true(cf, ncols, lane, [&](int c) { return colptr[c + 1] >= ce; });
#pragma unroll
  for (int t = 0; t < BUILD_CHUNK / 64; ++t) {
    const int i = cs + t * 64 + lane;
    if (i < ce) {
      const int r = rows[i];
      int lo = cf;
      if (nin < 64) {
        for (int j = 0; j < nin; ++j) lo += (i >= __builtin_amdgcn_readlane(e, j)) ? 1 : 0;
      } else {
        int hi = cl;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (colptr[mid] <= i) lo = mid; else hi = mid - 1;
        }
      }
      const double inv = 1.0 / (double)(fullrowptr[r + 1] - fullrowptr[r]);
      out_val[i] = (float)(inv * (double)normfact[lo]);
    }
  }
}

// COO index image of a CSR: indices[0][i] = row(i), indices[1][i] = col[i].
__global__ __launch_bounds__(256) void csr_to_coo_indices_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, int nrows, int64_t nnz,
    int64_t* __restrict__ indices) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nrows) return;
  const int b = rowptr[r];
  const int e = rowptr[r + 1];
  for (int i = b + lane; i < e; i += 64) {
    indices[i] = r;
    indices[nnz + i] = col[i];
  }
}

// Sorted COO rows -> CSR row pointer by gap filling (thread i owns rows (row[i-1], row[i]]).
__global__ __launch_bounds__(256) void coo_rowptr_kernel(const int64_t* __restrict__ row, int64_t nnz,
                                                         int M, int* __restrict__ rowptr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > nnz) return;
  const int64_t prev = (i == 0) ? -1 : row[i - 1];
  const int64_t cur = (i == nnz) ? (int64_t)M : row[i];
  for (int64_t k = prev + 1; k <= cur; ++k) rowptr[k] = (int)i;
}

__global__ __launch_bounds__(256) void narrow_index_kernel(const int64_t* __restrict__ in, int64_t n,
                                                           int* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (int)in[i];
}

// ---------------------------------------------------------------------------------
// Exclusive scan of n int32 counts into out[0..n] (out[n] = total), one workgroup.
// Optionally also writes the exclusive prefix into out2[0..n-1] (transpose cursors).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void scan_exclusive_kernel(const int* __restrict__ in, int n,
                                                              int* __restrict__ out,
                                                              int* __restrict__ out2) {
  constexpr int ITEMS = 8;
  __shared__ int wsum[16];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += 1024 * ITEMS) {
    int v[ITEMS];
    int tsum = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int idx = base + tid * ITEMS + k;
      v[k] = (idx < n) ? in[idx] : 0;
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
      int w = (lane < 16) ? wsum[lane] : 0;
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) {
        const int y = __shfl_up(w, d);
        if (lane >= d) w += y;
      }
      if (lane < 16) wsum[lane] = w;
    }
    __syncthreads();
    int excl = carry + (wave ? wsum[wave - 1] : 0) + x - tsum;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int idx = base + tid * ITEMS + k;
      if (idx < n) {
        out[idx] = excl;
        if (out2) out2[idx] = excl;
      }
      excl += v[k];
    }
    carry += wsum[15];
    __syncthreads();
  }
  if (tid == 0) out[n] = carry;
}

// ---------------------------------------------------------------------------------
// Transpose helpers.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void col_count_kernel(const int* __restrict__ col, int64_t nnz,
                                                        int* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nnz) atomicAdd(&cnt[col[i]], 1);
}

// Wave per source row: each entry claims a slot in its column's output row. The slot
// order inside an output row is arbitrary here; segsort restores ascending row order.
__global__ __launch_bounds__(256) void transpose_scatter_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val,
    int M, int* __restrict__ cursor, int* __restrict__ tr_col, float* __restrict__ tr_val) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= M) return;
  const int b = rowptr[r];
  const int e = rowptr[r + 1];
  for (int i = b + lane; i < e; i += 64) {
    const int pos = atomicAdd(&cursor[col[i]], 1);
    tr_col[pos] = r;
    tr_val[pos] = val[i];
  }
}

// ---------------------------------------------------------------------------------
// Tiled transpose (K <= TR_MAX_K): a stable counting sort by column with no global atomics
// and no sort pass. The nonzeros are cut into T tiles of TS consecutive entries (CSR order).
//  1. tr_tile_hist:   per tile, an LDS histogram of its columns -> hist[t][0..K).
//  2. tr_col_prefix:  per column, exclusive prefix of hist over tiles (in place) -> the
//                     offset of tile t's first entry inside output row c; totals -> cnt.
//     (then scan_exclusive_kernel turns cnt into tr_rowptr.)
//  3. tr_tile_scatter: per tile, LDS cursors cur[c] = tr_rowptr[c] + hist[t][c]; ONE wave
//                     walks the tile's rows in order, one row segment per LDS access, so
//                     the lanes of an access hold distinct columns and rows are placed in
//                     ascending order: the result is the canonical (coalesced) transpose.
// ---------------------------------------------------------------------------------
constexpr int TR_MAX_K = 32 * 1024;   // cursor / histogram array in LDS (128 KiB)
constexpr int TR_MAX_TS = 4 * 1024;   // tile entries preloaded in LDS (32 KiB)

__global__ __launch_bounds__(256) void tr_tile_hist_kernel(const int* __restrict__ col, int nnz, int TS, int K,
                                                           int* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) int lds_i[];
  const int t = blockIdx.x;
  for (int c = threadIdx.x; c < K; c += 256) lds_i[c] = 0;
  __syncthreads();
  const int b = t * TS;
  const int e = min(b + TS, nnz);
  for (int i = b + threadIdx.x; i < e; i += 256) atomicAdd(&lds_i[col[i]], 1);
  __syncthreads();
  int* h = hist + (int64_t)t * K;
  for (int c = threadIdx.x; c < K; c += 256) h[c] = lds_i[c];
}

__global__ __launch_bounds__(256) void tr_col_prefix_kernel(int* __restrict__ hist, int T, int K,
                                                            int* __restrict__ cnt) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= K) return;
  int run = 0;
  int t = 0;
  for (; t + 4 <= T; t += 4) {
    const int64_t o = (int64_t)t * K + c;
    const int h0 = hist[o], h1 = hist[o + K], h2 = hist[o + 2 * (int64_t)K], h3 = hist[o + 3 * (int64_t)K];
    hist[o] = run;
    hist[o + K] = run + h0;
    hist[o + 2 * (int64_t)K] = run + h0 + h1;
    hist[o + 3 * (int64_t)K] = run + h0 + h1 + h2;
    run += h0 + h1 + h2 + h3;
  }
  for (; t < T; ++t) {
    const int64_t o = (int64_t)t * K + c;
    const int h = hist[o];
    hist[o] = run;
    run += h;
  }
  cnt[c] = run;
}

__global__ __launch_bounds__(256) void tr_tile_scatter_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val, int M, int nnz,
    int TS, int K, const int* __restrict__ hist, const int* __restrict__ tr_rowptr, int* __restrict__ tr_col,
    float* __restrict__ tr_val) {
  // LDS: cur[K] cursors, then the tile's columns and values (preloaded by all 4 waves so
  // the ordered walk below reads only LDS and registers).
  extern __shared__ __attribute__((aligned(16))) int cur[];
  int* tcol = cur + ((K + 3) & ~3);
  float* tval = reinterpret_cast<float*>(tcol + TS);
  const int t = blockIdx.x;
  const int b = t * TS;
  const int e = min(b + TS, nnz);
  const int* h = hist + (int64_t)t * K;
  for (int c = threadIdx.x; c < K; c += 256) cur[c] = tr_rowptr[c] + h[c];
  for (int i = b + threadIdx.x; i < e; i += 256) {
    tcol[i - b] = col[i];
    tval[i - b] = val[i];
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  // first row with an entry at position >= b; row ends rowptr[r+1..r+64] held in a register
  int r = wave_first_true(0, M, lane, [&](int rr) { return rowptr[rr + 1] > b; });
  int wbase = r;
  int rp = rowptr[min(r + 1 + lane, M)];
  for (int base = b; base < e; base += 64) {
    const int i = base + lane;
    const bool valid = i < e;
    const int c = valid ? tcol[i - b] : 0;
    const float v = valid ? tval[i - b] : 0.0f;
    const int last = min(base + 64, e);  // one past the chunk's last entry
    bool todo = valid;
    while (true) {
      if (r - wbase >= 64) {
        wbase = r;
        rp = rowptr[min(r + 1 + lane, M)];
      }
      const int rend = readlane_i(rp, r - wbase);  // rowptr[r + 1], wave-uniform
      const bool mine = todo && i < rend;
      if (mine) {
        const int p = cur[c];
        cur[c] = p + 1;
        tr_col[p] = r;
        tr_val[p] = v;
      }
      todo = todo && !mine;
      if (rend >= last) break;  // row r continues into (or ends at) the next chunk
      ++r;
    }
  }
}

// ---------------------------------------------------------------------------------
// Segmented sort, ascending by int32 key with an fp32 payload, in place.
// Bitonic network in its "all comparators ascending" form (first step of every merge
// compares mirrored positions), so positions >= L can be treated as +inf and skipped.
// Segments: <=64 in registers, <=512 in a per-wave LDS region, <=16384 by one 1024-thread
// workgroup in LDS, longer ones by one workgroup in global memory. (Helpers: above the
// operand builder, which uses the same network.)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void segsort_wave_kernel(const int* __restrict__ ptr, int nseg,
                                                           int* __restrict__ key, float* __restrict__ val,
                                                           int* __restrict__ counters,
                                                           int* __restrict__ list_mid,
                                                           int* __restrict__ list_long) {
  __shared__ int sk[4][SEG_WAVE_LDS];
  __shared__ float sv[4][SEG_WAVE_LDS];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int s = blockIdx.x * 4 + w;
  if (s >= nseg) return;
  const int b = ptr[s];
  const int L = ptr[s + 1] - b;
  if (L <= 1) return;
  // already ascending?
  bool bad = false;
  for (int i = lane; i + 1 < L; i += 64) bad |= key[b + i] > key[b + i + 1];
  if (__ballot(bad) == 0ull) return;

  if (L <= 64) {
    int k = (lane < L) ? key[b + lane] : INT_MAX;
    float v = (lane < L) ? val[b + lane] : 0.0f;
    for (int size = 2; size <= 64; size <<= 1) {
      cmpx_reg(k, v, lane, size - 1);
      for (int d = size >> 2; d >= 1; d >>= 1) cmpx_reg(k, v, lane, d);
    }
    if (lane < L) {
      key[b + lane] = k;
      val[b + lane] = v;
    }
    return;
  }
  if (L <= SEG_WAVE_LDS) {
    int n = 1;
    while (n < L) n <<= 1;
    for (int i = lane; i < n; i += 64) {
      sk[w][i] = (i < L) ? key[b + i] : INT_MAX;
      sv[w][i] = (i < L) ? val[b + i] : 0.0f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int size = 2; size <= n; size <<= 1) {
      for (int d = size >> 1; d >= 1; d >>= 1) {
        const bool flip = (d == (size >> 1));
        for (int p = lane; p < (n >> 1); p += 64) {
          int i, j;
          bitonic_pair(p, size, d, flip, i, j);
          const int ki = sk[w][i], kj = sk[w][j];
          if (kj < ki) {
            const float vi = sv[w][i], vj = sv[w][j];
            sk[w][i] = kj;
            sk[w][j] = ki;
            sv[w][i] = vj;
            sv[w][j] = vi;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
    for (int i = lane; i < L; i += 64) {
      key[b + i] = sk[w][i];
      val[b + i] = sv[w][i];
    }
    return;
  }
  if (lane == 0) {
    if (L <= SEG_BLOCK_LDS) {
      list_mid[atomicAdd(&counters[0], 1)] = s;
    } else {
      list_long[atomicAdd(&counters[1], 1)] = s;
    }
  }
}

__global__ __launch_bounds__(1024) void segsort_block_kernel(const int* __restrict__ ptr,
                                                             int* __restrict__ key, float* __restrict__ val,
                                                             const int* __restrict__ counters,
                                                             const int* __restrict__ list) {
  __shared__ int sk[SEG_BLOCK_LDS];
  __shared__ float sv[SEG_BLOCK_LDS];
  const int count = counters[0];
  for (int t = blockIdx.x; t < count; t += gridDim.x) {
    const int s = list[t];
    const int b = ptr[s];
    const int L = ptr[s + 1] - b;
    int n = 1;
    while (n < L) n <<= 1;
    for (int i = threadIdx.x; i < n; i += 1024) {
      sk[i] = (i < L) ? key[b + i] : INT_MAX;
      sv[i] = (i < L) ? val[b + i] : 0.0f;
    }
    __syncthreads();
    for (int size = 2; size <= n; size <<= 1) {
      for (int d = size >> 1; d >= 1; d >>= 1) {
        const bool flip = (d == (size >> 1));
        for (int p = threadIdx.x; p < (n >> 1); p += 1024) {
          int i, j;
          bitonic_pair(p, size, d, flip, i, j);
          const int ki = sk[i], kj = sk[j];
          if (kj < ki) {
            const float vi = sv[i], vj = sv[j];
            sk[i] = kj;
            sk[j] = ki;
            sv[i] = vj;
            sv[j] = vi;
          }
        }
        __syncthreads();
      }
    }
    for (int i = threadIdx.x; i < L; i += 1024) {
      key[b + i] = sk[i];
      val[b + i] = sv[i];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(1024) void segsort_global_kernel(const int* __restrict__ ptr,
                                                              int* __restrict__ key, float* __restrict__ val,
                                                              const int* __restrict__ counters,
                                                              const int* __restrict__ list) {
  const int count = counters[1];
  for (int t = blockIdx.x; t < count; t += gridDim.x) {
    const int s = list[t];
    const int b = ptr[s];
    const int L = ptr[s + 1] - b;
    int64_t n = 1;
    while (n < L) n <<= 1;
    int* K = key + b;
    float* Vv = val + b;
    for (int64_t size = 2; size <= n; size <<= 1) {
      for (int64_t d = size >> 1; d >= 1; d >>= 1) {
        const bool flip = (d == (size >> 1));
        for (int64_t p = threadIdx.x; p < (n >> 1); p += 1024) {
          int64_t i, j;
          if (flip) {
            const int64_t half = size >> 1;
            i = (p / half) * size + (p % half);
            j = i ^ (size - 1);
          } else {
            i = (p / d) * (2 * d) + (p % d);
            j = i + d;
          }
          if (j < L) {
            const int ki = K[i], kj = K[j];
            if (kj < ki) {
              const float vi = Vv[i], vj = Vv[j];
              K[i] = kj;
              K[j] = ki;
              Vv[i] = vj;
              Vv[j] = vi;
            }
          }
        }
        __syncthreads();
      }
    }
  }
}

void tr_tiles(int64_t nnz, int64_t& TS, int64_t& T) {
  TS = ceil_div(nnz, 256);
  if (TS < 1024) TS = 1024;
  if (TS > TR_MAX_TS) TS = TR_MAX_TS;
  T = nnz > 0 ? ceil_div(nnz, TS) : 0;
}

size_t segsort_ws(int64_t nseg) { return 256 + align_up((size_t)(nseg > 0 ? nseg : 1) * 4, 256) * 2; }

struct SegLists {
  int* counters;
  int* list_mid;
  int* list_long;
};

SegLists seg_lists(void* ws, int64_t nseg) {
  char* w = (char*)ws;
  return SegLists{(int*)w, (int*)(w + 256), (int*)(w + 256 + align_up((size_t)(nseg > 0 ? nseg : 1) * 4, 256))};
}

// Sort the queued segments: the workgroup (LDS) sorter for counters[0] entries, the
// global-memory sorter for counters[1]. Small grids: they loop over the (usually empty)
// lists, reading the counts on the device (no host synchronisation).
int run_list_sorters(const int* ptr, int* key, float* val, const SegLists& l, hipStream_t st) {
  segsort_block_kernel<<<dim3(16), dim3(1024), 0, st>>>(ptr, key, val, l.counters, l.list_mid);
  GNN_LAUNCHED("segsort_block_kernel");
  segsort_global_kernel<<<dim3(4), dim3(1024), 0, st>>>(ptr, key, val, l.counters, l.list_long);
  GNN_LAUNCHED("segsort_global_kernel");
  return 0;
}

int run_segsort(const int* ptr, int64_t nseg, int* key, float* val, void* ws, hipStream_t st) {
  if (nseg <= 0) return 0;
  const SegLists l = seg_lists(ws, nseg);
  GNN_HIP(hipMemsetAsync(l.counters, 0, 16, st), "segsort counters memset");
  segsort_wave_kernel<<<dim3((unsigned)ceil_div(nseg, 4)), dim3(256), 0, st>>>(ptr, (int)nseg, key, val, l.counters,
                                                                            l.list_mid, l.list_long);
  GNN_LAUNCHED("segsort_wave_kernel");
  return run_list_sorters(ptr, key, val, l, st);
}

int build_operand(const int32_t* fullrowptr, const int32_t* rowptr, const void* colidx, int colidx_bytes,
                  const float* normfact, int64_t nrows, int64_t ncols, int64_t nnz, int32_t* csr_col, float* csr_val,
                  int64_t* coo_indices, unsigned long long* flag, void* stream) {
  // flag == nullptr: rows guaranteed column-ascending (no check, no fix pass)
  GNN_REQUIRE(nrows >= 0 && ncols >= 0 && nnz >= 0, "gnn_build_operand_f32: negative size");
  GNN_REQUIRE(nrows < INT_MAX && ncols < INT_MAX && nnz < INT_MAX, "gnn_build_operand_f32: sizes must be < 2^31");
  GNN_REQUIRE(colidx_bytes == 2 || colidx_bytes == 4 || colidx_bytes == 8,
              "gnn_build_operand_f32: colidx_bytes must be 2, 4 or 8 (got %d)", colidx_bytes);
  if (nrows == 0 || nnz == 0) return 0;
  GNN_REQUIRE(fullrowptr && rowptr && colidx && normfact && csr_col && csr_val, "gnn_build_operand_f32: NULL input");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(nrows, 4));
  const bool sorted = flag == nullptr;
  const unsigned long long gen = 1;
  if (!sorted) GNN_HIP(hipMemsetAsync(flag, 0, 2 * sizeof(*flag), st), "operand flag memset");
  const dim3 gflat((unsigned)ceil_div(nnz, 4 * BUILD_CHUNK));  // 4 waves x BUILD_CHUNK nonzeros
  const dim3 gfix(16);  // usually a no-op (gated): keep the launch small
  auto build = [&](auto* ci) {  // ci: colidx in its own width
    build_operand_flat_kernel<<<gflat, dim3(256), 0, st>>>(fullrowptr, rowptr, ci, normfact, (int)nrows, (int)nnz,
                                                            csr_col, csr_val, flag, gen);
    GNN_LAUNCHED("build_operand_flat_kernel");
    if (!sorted)
      build_operand_kernel<<<gfix, dim3(256), 0, st>>>(fullrowptr, rowptr, ci, normfact, (int)nrows, csr_col, csr_val,
                                                        flag, gen);
    GNN_LAUNCHED("build_operand_kernel");
    return 0;
  };
  const int rc = colidx_bytes == 2   ? build((const int16_t*)colidx)
                 : colidx_bytes == 4 ? build((const int32_t*)colidx)
                                     : build((const int64_t*)colidx);
  if (rc) return rc;
  if (coo_indices) {
    csr_to_coo_indices_kernel<<<grid, dim3(256), 0, st>>>(rowptr, csr_col, (int)nrows, nnz, coo_indices);
    GNN_LAUNCHED("csr_to_coo_indices_kernel");
  }
  return 0;
}
}  // namespace

int gnn::launch_scan_exclusive(const int* in, int n, int* out, hipStream_t st) {
  scan_exclusive_kernel<<<dim3(1), dim3(1024), 0, st>>>(in, n, out, nullptr);
  GNN_LAUNCHED("scan_exclusive_kernel");
  return 0;
}

extern "C" {

size_t gnn_segsort_workspace_bytes(int64_t nseg) { return segsort_ws(nseg); }

size_t gnn_build_operand_workspace_bytes(void) { return 256; }

int gnn_build_operand_f32(const int32_t* fullrowptr, const int32_t* rowptr, const void* colidx, int colidx_bytes,
                          const float* normfact, int64_t nrows, int64_t ncols, int64_t nnz, int32_t* csr_col,
                          float* csr_val, int64_t* coo_indices, void* workspace, size_t workspace_bytes,
                          void* stream) {
  // the "unsorted row seen" and "repeated column seen" words live in the caller's workspace,
  // zeroed on the call's stream: no allocation inside the library, no state shared between
  // concurrent calls
  GNN_REQUIRE(nrows == 0 || nnz == 0 || (workspace != nullptr && workspace_bytes >= 16 && (uintptr_t)workspace % 8 == 0),
              "gnn_build_operand_f32: needs an 8-byte aligned workspace of gnn_build_operand_workspace_bytes() bytes");
  return build_operand(fullrowptr, rowptr, colidx, colidx_bytes, normfact, nrows, ncols, nnz, csr_col, csr_val,
                       coo_indices, (unsigned long long*)workspace, stream);
}

int gnn_build_operand_sorted_f32(const int32_t* fullrowptr, const int32_t* rowptr, const void* colidx,
                                 int colidx_bytes, const float* normfact, int64_t nrows, int64_t ncols, int64_t nnz,
                                 int32_t* csr_col, float* csr_val, int64_t* coo_indices, void* stream) {
  return build_operand(fullrowptr, rowptr, colidx, colidx_bytes, normfact, nrows, ncols, nnz, csr_col, csr_val,
                       coo_indices, nullptr, stream);
}

int gnn_build_operand_t_f32(const int32_t* fullrowptr, const int32_t* colptr, const int32_t* rows,
                            const float* normfact, int64_t nrows, int64_t ncols, int64_t nnz, float* val_t,
                            void* stream) {
  GNN_REQUIRE(nrows >= 0 && ncols >= 0 && nnz >= 0, "gnn_build_operand_t_f32: negative size");
  GNN_REQUIRE(nrows < INT_MAX && ncols < INT_MAX && nnz < INT_MAX, "gnn_build_operand_t_f32: sizes must be < 2^31");
  if (ncols == 0 || nnz == 0) return 0;
  GNN_REQUIRE(fullrowptr && colptr && rows && normfact && val_t, "gnn_build_operand_t_f32: NULL input");
  build_operand_t_kernel<<<dim3((unsigned)ceil_div(nnz, 4 * BUILD_CHUNK)), dim3(256), 0, (hipStream_t)stream>>>(
      fullrowptr, colptr, rows, normfact, (int)ncols, (int)nnz, val_t);
  GNN_LAUNCHED("build_operand_t_kernel");
  return 0;
}

int gnn_coo_to_csr(const int64_t* row, const int64_t* col, int64_t nnz, int64_t M, int32_t* rowptr, int32_t* col32,
                   void* stream) {
  GNN_REQUIRE(nnz >= 0 && M >= 0, "gnn_coo_to_csr: negative size");
  GNN_REQUIRE(nnz < INT_MAX && M < INT_MAX, "gnn_coo_to_csr: sizes must be < 2^31");
  GNN_REQUIRE(rowptr != nullptr, "gnn_coo_to_csr: NULL rowptr");
  GNN_REQUIRE(nnz == 0 || row != nullptr, "gnn_coo_to_csr: NULL row");
  hipStream_t st = (hipStream_t)stream;
  coo_rowptr_kernel<<<dim3((unsigned)ceil_div(nnz + 1, 256)), dim3(256), 0, st>>>(row, nnz, (int)M, rowptr);
  GNN_LAUNCHED("coo_rowptr_kernel");
  if (col32 && nnz > 0) {
    GNN_REQUIRE(col != nullptr, "gnn_coo_to_csr: NULL col");
    narrow_index_kernel<<<dim3((unsigned)ceil_div(nnz, 256)), dim3(256), 0, st>>>(col, nnz, col32);
    GNN_LAUNCHED("narrow_index_kernel");
  }
  return 0;
}

size_t gnn_csr_transpose_workspace_bytes(int64_t M, int64_t K, int64_t nnz) {
  (void)M;
  const size_t fallback = align_up((size_t)(K > 0 ? K : 1) * 4, 256) + segsort_ws(K);
  if (K > TR_MAX_K) return fallback;
  int64_t TS = 0, T = 0;
  tr_tiles(nnz, TS, T);
  const size_t tiled = align_up((size_t)T * (size_t)K * 4, 256) + align_up((size_t)(K > 0 ? K : 1) * 4, 256);
  return tiled > fallback ? tiled : fallback;
}

int gnn_csr_transpose(const int32_t* rowptr, const int32_t* col, const float* val, int64_t M, int64_t K, int64_t nnz,
                      int32_t* tr_rowptr, int32_t* tr_col, float* tr_val, void* workspace, size_t workspace_bytes,
                      void* stream) {
  GNN_REQUIRE(M >= 0 && K >= 0 && nnz >= 0, "gnn_csr_transpose: negative size");
  GNN_REQUIRE(M < INT_MAX && K < INT_MAX && nnz < INT_MAX, "gnn_csr_transpose: sizes must be < 2^31");
  GNN_REQUIRE(tr_rowptr != nullptr, "gnn_csr_transpose: NULL tr_rowptr");
  hipStream_t st = (hipStream_t)stream;
  if (K == 0) return 0;
  if (nnz == 0 || M == 0) {
    GNN_HIP(hipMemsetAsync(tr_rowptr, 0, (size_t)(K + 1) * 4, st), "transpose memset");
    return 0;
  }
  GNN_REQUIRE(rowptr && col && val && tr_col && tr_val, "gnn_csr_transpose: NULL input/output");
  GNN_REQUIRE(workspace && workspace_bytes >= gnn_csr_transpose_workspace_bytes(M, K, nnz),
              "gnn_csr_transpose: workspace too small");
  char* w = (char*)workspace;
  if (K <= TR_MAX_K) {
    int64_t TS = 0, T = 0;
    tr_tiles(nnz, TS, T);
    int* hist = (int*)w;
    int* cnt = (int*)(w + align_up((size_t)T * (size_t)K * 4, 256));
    const size_t lds = (size_t)K * 4;
    static bool attr_set = false;
    if (!attr_set) {
      GNN_HIP(hipFuncSetAttribute((const void*)tr_tile_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  TR_MAX_K * 4), "hipFuncSetAttribute(tr_tile_hist)");
      GNN_HIP(hipFuncSetAttribute((const void*)tr_tile_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  TR_MAX_K * 4 + TR_MAX_TS * 8), "hipFuncSetAttribute(tr_tile_scatter)");
      attr_set = true;
    }
    tr_tile_hist_kernel<<<dim3((unsigned)T), dim3(256), lds, st>>>(col, (int)nnz, (int)TS, (int)K, hist);
    GNN_LAUNCHED("tr_tile_hist_kernel");
    tr_col_prefix_kernel<<<dim3((unsigned)ceil_div(K, 256)), dim3(256), 0, st>>>(hist, (int)T, (int)K, cnt);
    GNN_LAUNCHED("tr_col_prefix_kernel");
    scan_exclusive_kernel<<<dim3(1), dim3(1024), 0, st>>>(cnt, (int)K, tr_rowptr, nullptr);
    GNN_LAUNCHED("scan_exclusive_kernel");
    const size_t lds3 = (size_t)((K + 3) & ~3) * 4 + (size_t)TS * 8;
    tr_tile_scatter_kernel<<<dim3((unsigned)T), dim3(256), lds3, st>>>(rowptr, col, val, (int)M, (int)nnz, (int)TS,
                                                                     (int)K, hist, tr_rowptr, tr_col, tr_val);
    GNN_LAUNCHED("tr_tile_scatter_kernel");
    return 0;
  }
  // Large K: atomic slot claim + segmented sort (also canonical and deterministic).
  int* cnt = (int*)w;
  void* ssws = w + align_up((size_t)K * 4, 256);
  GNN_HIP(hipMemsetAsync(cnt, 0, (size_t)K * 4, st), "transpose count memset");
  col_count_kernel<<<dim3((unsigned)ceil_div(nnz, 256)), dim3(256), 0, st>>>(col, nnz, cnt);
  GNN_LAUNCHED("col_count_kernel");
  scan_exclusive_kernel<<<dim3(1), dim3(1024), 0, st>>>(cnt, (int)K, tr_rowptr, cnt);
  GNN_LAUNCHED("scan_exclusive_kernel");
  transpose_scatter_kernel<<<dim3((unsigned)ceil_div(M, 4)), dim3(256), 0, st>>>(rowptr, col, val, (int)M, cnt,
                                                                               tr_col, tr_val);
  GNN_LAUNCHED("transpose_scatter_kernel");
  return run_segsort(tr_rowptr, K, tr_col, tr_val, ssws, st);
}

}  // extern "C"
