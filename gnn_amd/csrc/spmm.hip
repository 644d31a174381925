// spmm.hip — MI355X (gfx950, CDNA4) kernels and C ABI of the SpMM aggregation.
//
// What the reference does (spmm_cpp/cuda_spmm.cu:619-704): per call it converts the COO
// indices to int32, zero-fills Y, builds a row pointer and a "virtual row" split of every
// row into <=64-nnz chunks with a Blelloch scan (5-6 device syncs, 3 .item() reads, raw
// cudaMalloc/cudaFree), then runs one 32-thread half-block per virtual row that gathers
// X rows with scalar 4-byte loads and atomically adds each 64-column tile into Y.
//
// What this file does instead (design: DESIGN.md §Kernels):
//  * The operand is CSR (int32 rowptr/col, fp32 val), built once per sampled layer by
//    gnn_build_operand_f32 (operand.hip, the create_coo_tensor replacement) — no per-call
//    conversion.
//  * Load balance without a scan: the nonzeros are cut into fixed work units of S
//    consecutive entries (S = unit_nnz). One 64-lane wave owns one unit; it finds its
//    first/last row with a 64-way parallel search of rowptr and walks the rows in order.
//    A row of at most S nonzeros is owned whole by the unit holding its first nonzero and
//    stored straight to Y (empty rows store zeros, so Y is never memset); only longer rows
//    are cut at unit boundaries: their pieces go to a slab and a small second kernel adds
//    them in unit order. No atomics: results are deterministic.
//  * Inside a wave, G lanes span the feature columns with VW-wide (8 or 16 byte) loads,
//    NJ column chunks per lane, and the 64/G lane groups take different nonzeros of the
//    same row; U nonzeros are issued back to back so U*NJ row loads are in flight per lane
//    before the FMAs (memory-level parallelism for an HBM/Infinity-Cache bound gather).
//  * Everything is stream-ordered on the caller's stream: no host syncs, no allocation.
//
// The file holds the aggregation only: the unit, row and combine kernels, the two block kernels
// that make a block-local CSR of the resident graph, the host code that picks a configuration and
// a kernel for a call, and the gnn_spmm_* C ABI. Operands are built in operand.hip, features
// gathered in gather.hip, and the library's error state lives in runtime.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <utility>

#include "gnn_spmm.h"
#include "common.h"
#include "spmm_device.h"

namespace {

using gnn::align_up;
using gnn::ceil_div;
using gnn::pick_vw;

// ---------------------------------------------------------------------------------
// SpMM main kernel. One wave per work unit of S consecutive nonzeros.
//   VW: floats per load (1/2/4); G: lanes per column group (64/32/16); NJ: column chunks
//   per lane; U: nonzeros per lane group issued back to back.
// Column of chunk j for a lane: tile_base + (lane % G) * VW + j * G * VW.
// Slab layout: [nunits][2][ldslab]; slot 0 = piece of a row that began in an earlier unit,
// slot 1 = piece of a row that begins in this unit and continues past it.
// Empty rows are not walked by the nonzero units: ROW_UNIT-row "row units" appended to the
// grid store them (zeros, or the residual row). Left to the unit holding their position, a
// run of empty rows (a FastGCN layer's transpose: most of its 8 k rows) serialised on one
// wave — 54 us for a 17 MB output.
// ---------------------------------------------------------------------------------
constexpr int ROW_UNIT = 64;

// Workgroup -> (unit block, column tile). The launch is 1-D; workgroups are dealt to the 8
// XCDs round-robin (b and b + 8 share one, MI355X_MICROARCH.md §Workgroup dispatch), and
// each XCD has its own 4 MiB L2. In tile-major order (xcd_chunk == 0) all 8 XCDs sweep the
// same column tile at once, so every L2 must hold that tile's whole slice of X. With the
// XCD map the tile-major list of W = gx * tiles items is cut into 8 contiguous chunks of
// xcd_chunk items and workgroup b works on item (b % 8) * xcd_chunk + b / 8: each XCD walks
// its own chunk in order, i.e. its own tile at a time, and holds only that tile's slice.
struct WorkMap {
  int gx;         // unit blocks per column tile (incl. the row-unit blocks)
  int items;      // gx * tiles
  int xcd_chunk;  // 0: tile-major order; else ceil(items / 8)
  __device__ __forceinline__ bool locate(unsigned b, int& ub, int& tile) const {
    int w = (int)b;
    if (xcd_chunk) {
      w = (int)(b & 7u) * xcd_chunk + (int)(b >> 3);
      if (w >= items) return false;
    }
    tile = w / gx;
    ub = w - tile * gx;
    return true;
  }
};

// Element kind of X (GNN_FEAT_*). fp32 rows are loaded as the V the FMAs take. 16-bit rows (VW 4
// only) are loaded 4 elements at a time as two 32-bit words (8 bytes, global_load_dwordx2), kept as
// loaded until the FMAs and widened there in registers: bf16 is the upper half of the fp32 pattern
// (a shift / a mask of the word), fp16 the hardware convert of each half (fp16 denormals are on in
// gfx9 code objects), both exact — so the fmaf chain sees the values the fp32 kernel reads from the
// widened copy of X and gives the same bits. Two zero words widen to the fp32 zero vector the
// skipped slots use.
typedef unsigned int xw2 __attribute__((ext_vector_type(2)));
template <int XK, int VW> struct XLoad {
  using E = float;
  using T = typename Vec<VW>::T;
  static __device__ __forceinline__ T widen(T x) { return x; }
};
template <int VW> struct XLoad<GNN_FEAT_F16, VW> {
  static_assert(VW == 4, "16-bit X rows are read 4 elements per load");
  using E = unsigned short;
  using T = xw2;
  static __device__ __forceinline__ float half_of(unsigned w, int hi) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(hi ? w >> 16 : w & 0xffffu));
  }
  static __device__ __forceinline__ f4 widen(xw2 x) {
    return f4{half_of(x.x, 0), half_of(x.x, 1), half_of(x.y, 0), half_of(x.y, 1)};
  }
};
template <int VW> struct XLoad<GNN_FEAT_BF16, VW> {
  static_assert(VW == 4, "16-bit X rows are read 4 elements per load");
  using E = unsigned short;
  using T = xw2;
  static __device__ __forceinline__ f4 widen(xw2 x) {
    return f4{__uint_as_float(x.x << 16), __uint_as_float(x.x & 0xffff0000u), __uint_as_float(x.y << 16),
              __uint_as_float(x.y & 0xffff0000u)};
  }
};

// One column chunk per lane: held to 8 waves per SIMD (<= 64 VGPRs; the slot-skip branches
// below otherwise take 66); wider instantiations keep the compiler's choice (no spills).
// The body is spmm_unit_body.inc, shared as text with the 16-bit kernel below (a shared device
// function, inlined, changed the fp32 kernel's code: 50 -> 64 VGPRs for <4, 16, 1, 4, false>).
template <int VW, int G, int NJ, int U, bool RES>
__global__ __launch_bounds__(256, (NJ == 1 && U <= 4) ? 8 : 1) void spmm_unit_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val,
    int M, int nnz, int S, int nunits,
    const float* __restrict__ X, int64_t ldx,
    float* __restrict__ Y, int64_t ldy,
    float* __restrict__ slab, int64_t ldslab, int F,
    const float* __restrict__ R, int64_t ldr, const int* __restrict__ rmap, WorkMap wm) {
  constexpr int XK = GNN_FEAT_F32;
#include "spmm_unit_body.inc"
}

// The same walk over 16-bit X rows (KIND = GNN_FEAT_F16 / GNN_FEAT_BF16; ldx in elements), VW 4 and
// no residual: layer 0 aggregating straight from a 16-bit feature store's rows. Launched with the
// geometry of the fp32 call (G, NJ, tiles, S, WorkMap), it is bit-identical to it on widened X.
template <int KIND, int G, int NJ, int U>
__global__ __launch_bounds__(256, (NJ == 1 && U <= 4) ? 8 : 1) void spmm_unit16_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val,
    int M, int nnz, int S, int nunits,
    const unsigned short* __restrict__ X, int64_t ldx,
    float* __restrict__ Y, int64_t ldy,
    float* __restrict__ slab, int64_t ldslab, int F, WorkMap wm) {
  constexpr int XK = KIND, VW = 4;
  constexpr bool RES = false;
  const float* const R = nullptr;  // named by the body's discarded residual branches
  const int64_t ldr = 0;
  const int* const rmap = nullptr;
#include "spmm_unit_body.inc"
}

// Adds the unit pieces of every cut row (> S nonzeros), in unit order. A workgroup covers
// `rows` rows (<= 64): every wave loads their rowptr pairs at once (one dependent round, not one
// per row) and ballots the cut ones; the (cut row, 64*VW-column pass) items are dealt to the 4
// waves, so a cluster of long rows still spreads over the workgroup. 4 rows per workgroup (1 for
// operands under 512 rows): more, smaller workgroups finish sooner beside the concurrent staging
// kernels — combines per step 50.9 (16 rows) vs 45.4 (4 rows) vs 71.9 (32) us, and the layer-2
// forward's 10.7 -> 6.0 us (A/B/A/B under the bench, profiles/round3/spmm/combine_rows_*).
constexpr int COMBINE_ROWS = 4;
constexpr int COMBINE_LOADS = 4;  // pieces of a cut row loaded before they are added
int combine_rows(int64_t M) { return M >= 512 ? COMBINE_ROWS : 1; }

template <int VW, int COMBINE_BATCH>
__global__ __launch_bounds__(256) void spmm_combine_kernel(
    const int* __restrict__ rowptr, int M, int S,
    const float* __restrict__ slab, int64_t ldslab,
    float* __restrict__ Y, int64_t ldy, int F,
    const float* __restrict__ R, int64_t ldr, const int* __restrict__ rmap, int rows) {
  using V = typename Vec<VW>::T;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int r0 = blockIdx.x * rows;
  const int rl = r0 + lane;
  const bool is_cut = lane < rows && rl < M && (rowptr[rl + 1] - rowptr[rl]) > S;  // ownership rule
  const unsigned long long cutmask = __ballot(is_cut);
  if (cutmask == 0ull) return;
  const int npass = (F + 64 * VW - 1) / (64 * VW);
  const int items = __builtin_popcountll(cutmask) * npass;
  for (int it = w; it < items; it += 4) {
    unsigned long long m = cutmask;
    for (int k = it / npass; k > 0; --k) m &= m - 1;  // the (it / npass)-th cut row
    const int r = r0 + __builtin_ctzll(m);
    const int cc = (it % npass) * 64 * VW + lane * VW;
    if (cc >= F) continue;
    const int rb = rowptr[r];
    const int re = rowptr[r + 1];
    const int u0 = rb / S;
    const int u1 = (re - 1) / S;
    const int q = rmap ? rmap[r] : -1;
    {
      // pieces in unit order: slot 1 of u0, then slot 0 of u0 + 1 .. u1, added in that order,
      // COMBINE_BATCH pieces' loads in flight at once (A/B of 2 / 4 / 8 / 16 under the bench,
      // profiles/round3/spmm/combine_loads_r3ar_r3as/: 4 and 8 equal, 2 and 16 slower)
      const int np = u1 - u0 + 1;  // wave-uniform
      V s = vzero<VW>();
      for (int b = 0; b < np; b += COMBINE_BATCH) {
        V a[COMBINE_BATCH];
#pragma unroll
        for (int k = 0; k < COMBINE_BATCH; ++k) {
          const int p = b + k;
          if (p < np) a[k] = *reinterpret_cast<const V*>(slab + ((int64_t)(u0 + p) * 2 + (p == 0 ? 1 : 0)) * ldslab + cc);
        }
#pragma unroll
        for (int k = 0; k < COMBINE_BATCH; ++k) {
          const int p = b + k;
          if (p < np) s = p == 0 ? a[k] : s + a[k];
        }
      }
      if (q >= 0) s += *reinterpret_cast<const V*>(R + (int64_t)q * ldr + cc);
      *reinterpret_cast<V*>(Y + (int64_t)r * ldy + cc) = s;
    }
  }
}

// ---------------------------------------------------------------------------------
// Small operands (the layer-2 calls: 15 k nonzeros, F = 1024): one workgroup of WPR waves per
// (row, column slice of 64 * VW * NJ floats), no work units, no slab, no combine launch.
// The unit kernel's parallelism comes from many equal units; on a 15 k-entry operand it has a
// few thousand short waves, each a chain of dependent loads (row search, (col, val), gathers
// in rounds of U, store) with 4 row loads in flight: 24-25 us per call + a combine launch for
// the cut rows, latency-bound. Here a wave owns one row (WPR = 1) or a contiguous 1/WPR of it
// (long rows: the layer-2 forward's 512 rows reach 484 nonzeros), issues U row loads per lane
// before its FMAs, and the WPR partial rows are added in wave order through LDS by wave 0.
// WPR = 1: every output element is a C fmaf chain over the row in CSR order (bit-identical to
// the oracle); WPR > 1: WPR such chains added in order (deterministic). Empty rows store zeros
// (or the residual row).
// ---------------------------------------------------------------------------------

template <int VW, int NJ, int U, int WPR, bool RES>
__global__ __launch_bounds__(64 * WPR) void spmm_row_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val, int M,
    const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int F, int slices,
    const float* __restrict__ R, int64_t ldr, const int* __restrict__ rmap) {
  constexpr int XK = GNN_FEAT_F32;
#include "spmm_row_body.inc"
}

// 16-bit X rows (see spmm_unit16_kernel): VW 4, no residual.
template <int KIND, int NJ, int U, int WPR>
__global__ __launch_bounds__(64 * WPR) void spmm_row16_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val, int M,
    const unsigned short* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int F, int slices) {
  constexpr int XK = KIND, VW = 4;
  constexpr bool RES = false;
  const float* const R = nullptr;
  const int64_t ldr = 0;
  const int* const rmap = nullptr;
#include "spmm_row_body.inc"
}

// Row pointer and values of rows [row0, row0 + rows) of the resident graph as a block-local CSR
// (gnn_spmm_graph_f32): rowptr[i] = indptr[row0 + i] - e0, val[e] = (float)(1.0 / degree(row)) —
// build_operand_kernel's value with normfact = 1. One wave per row (wave `rows` writes the end).
// The pointer is clamped to [0, nnz] and its two ends are pinned to 0 and nnz, so a device
// indptr that disagrees with the host's e0 / nnz still gives the aggregation a row pointer whose
// every entry indexes inside the block's nnz columns and values (wrong sums, no stray access).
__global__ __launch_bounds__(256) void graph_block_kernel(
    const int64_t* __restrict__ indptr, const int* __restrict__ degree, int64_t row0, int rows, int64_t e0,
    int nnz, int* __restrict__ rowptr, float* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int64_t i64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i64 > rows) return;
  const int i = (int)i64;
  if (i == rows) {
    if (lane == 0) rowptr[rows] = nnz;
    return;
  }
  const int64_t lo = indptr[row0 + i] - e0;
  const int64_t hi = indptr[row0 + i + 1] - e0;
  const int b = i == 0 ? 0 : (int)min(max(lo, (int64_t)0), (int64_t)nnz);
  const int e = i == rows - 1 ? nnz : (int)min(max(hi, (int64_t)0), (int64_t)nnz);
  if (lane == 0) rowptr[i] = b;
  if (b >= e) return;
  const float w = (float)(1.0 / (double)degree[row0 + i]);
  for (int64_t k = (int64_t)b + lane; k < e; k += 64) val[k] = w;
}

// Block-local CSR of the graph rows rows[0..M) with the columns relabelled to positions in a node
// set (gnn_spmm_rows_f32): rowptr from the host's degree scan rowseg, clamped and pinned as above;
// col[e] = the position of the entry's column in the set of the membership table tab (closure.hip /
// extract.hip's word: x = the bits of 32 node ids, y = the members below them; one 8-byte load per
// entry), val[e] = (float)(1.0 / degree(row)). One wave per row, its entries over the lanes (wave M
// writes the end). Every entry position below nnz is written by exactly one row (consecutive rows
// share their clamped bound), and an entry that cannot be resolved — a column outside the set or
// not below K, a row id outside the graph, a scan that gives the row more entries than the graph
// holds — is stored as column 0 with value 0 and raises err bit 0: the aggregation reads X rows
// below K whatever the inputs hold.
__global__ __launch_bounds__(256) void rows_block_kernel(
    const int64_t* __restrict__ indptr, const int* __restrict__ indices, const int* __restrict__ degree,
    int num_nodes, const int* __restrict__ rows, int M, const int* __restrict__ rowseg, int nnz,
    const uint2* __restrict__ tab, int K, int* __restrict__ rowptr, int* __restrict__ col, float* __restrict__ val,
    int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t i64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i64 > M) return;
  const int i = (int)i64;
  if (i == M) {
    if (lane == 0) rowptr[M] = nnz;
    return;
  }
  const int b = i == 0 ? 0 : min(max(rowseg[i], 0), nnz);
  const int e = i == M - 1 ? nnz : min(max(rowseg[i + 1], 0), nnz);
  if (lane == 0) rowptr[i] = b;
  if (b >= e) return;
  const int r = rows[i];
  const bool inside = (unsigned)r < (unsigned)num_nodes;
  const int64_t src = inside ? indptr[r] : 0;
  const int64_t len = inside ? indptr[r + 1] - src : 0;
  const float w = inside ? (float)(1.0 / (double)degree[r]) : 0.0f;
  bool bad = false;
  for (int64_t k = (int64_t)b + lane; k < e; k += 64) {
    const int64_t j = k - b;
    int p = -1;
    if (j < len) {
      const int c = indices[src + j];
      if ((unsigned)c < (unsigned)num_nodes) {
        const uint2 wd = tab[c >> 5];
        const unsigned sh = (unsigned)c & 31u;
        if ((wd.x >> sh) & 1u) p = (int)wd.y + __builtin_popcount(wd.x & ((1u << sh) - 1u));
      }
    }
    const bool ok = p >= 0 && p < K;
    col[k] = ok ? p : 0;
    val[k] = ok ? w : 0.0f;
    bad |= !ok;
  }
  if (err && bad) atomicOr(err, 1);
}

// ---------------------------------------------------------------------------------
// Host-side configuration and dispatch.
// ---------------------------------------------------------------------------------
struct SpmmCfg {
  int vw, g, nj, tiles;
  int64_t unit, nunits, ldslab;
  // small operands: spmm_row_kernel<vw, rnj, ru, wpr> over M * slices workgroups (wpr == 0: the
  // unit kernel above)
  int wpr, rnj, ru, slices;
  // small operands cut into 256-float column tiles (small_tiles): 16 nonzeros in flight per lane
  // instead of 4 (their units are short chains of latency-bound rounds)
  bool u16;
};

// The row kernel takes operands whose nonzeros are too few to fill the chip with units: up to
// ROWK_MAX_NNZ nonzeros and ROWK_MAX_WG workgroups (GNN_SPMM_ROWK=0 / 1 forces it off / on when
// the caller did not fix the unit size).
constexpr int64_t ROWK_MAX_NNZ = 65536;
constexpr int64_t ROWK_MAX_WG = 1 << 20;

void pick_row_kernel(SpmmCfg& c, int64_t M, int64_t nnz, int64_t F, int64_t unit) {
  c.wpr = 0;
  if (unit > 0 || M <= 0 || F <= 0) return;  // a fixed unit size asks for the unit kernel
  const char* env = getenv("GNN_SPMM_ROWK");
  const int mode = env ? atoi(env) : -1;
  if (mode == 0) return;
  const int64_t chunks = ceil_div(F, (int64_t)64 * c.vw);  // 64-lane column chunks covering F
  // many rows: whole rows per wave, up to 4 chunks per lane; few rows: one chunk per slice
  int nj = 1;
  if (c.vw == 4 && M >= 4096) nj = chunks >= 4 ? 4 : (chunks >= 2 ? 2 : 1);
  const int64_t slices = ceil_div(chunks, (int64_t)nj);
  const double avg = (double)nnz / (double)M;
  // Measured on the layer-2 calls (profiles/round4/layer2/): short rows (the backward's Aᵀ, 1.7
  // nonzeros per row) 12.7-13.7 us with 1-2 waves per row against 25 us for units + combine;
  // long-tailed rows (the forward's A, 29 per row, up to 484) 20.4 us at best (8 waves per row)
  // against 19.5 for units + combine — so by default only short-row operands take this kernel,
  // with one wave per row (each output a C fmaf chain: the executor folds such a call into the
  // tail that consumes it, gnn_sage_norm_bwd_agg_f32, bit for bit).
  // (round 5: a dynamic form, one wave per 8 nonzeros of a row up to 16 per workgroup, took the
  // layer-2 forward to 49 us in the step against 23 for units + combine: not kept)
  if (mode != 1 && avg >= 12.0) return;
  int wpr = avg >= 48.0 ? 8 : (avg >= 12.0 ? 4 : 1);
  if (const char* e = getenv("GNN_SPMM_ROWK_WPR")) {  // experiments
    const int v = atoi(e);
    if (v == 1 || v == 2 || v == 4 || v == 8) wpr = v;
  }
  if (mode != 1 && (nnz > ROWK_MAX_NNZ || M * slices > ROWK_MAX_WG)) return;
  if (M * slices >= (int64_t)INT_MAX) return;
  c.wpr = wpr;
  c.rnj = nj;
  c.ru = nj == 1 ? 16 : (nj == 2 ? 8 : 4);
  c.slices = (int)slices;
}

// About 2.4 rows' worth of nonzeros as a power of two in [16, 256] (see default_unit).
int64_t row_unit(int64_t M, int64_t nnz) {
  int64_t s = 256;
  if (M > 0) {
    const double want = 2.4 * (double)nnz / (double)M;
    while (s > 16 && (double)s > want * 1.41421356) s >>= 1;
  }
  return s;
}

// Small operands (fewer than 2048 row-sized units) take their parallelism from 256-float
// column tiles before cutting rows into pieces: the layer-2 forward (512 rows of ~30
// nonzeros, F = 1024) had 2048 units of 8 nonzeros, every row cut and recombined (14 + 17 us).
// (Operands with < 16 nonzeros per row keep their two-rows-per-unit path.)
int64_t small_tiles(int64_t M, int64_t nnz, int64_t F) {
  if (F < 512 || nnz <= 0 || nnz < 16 * M || ceil_div(nnz, row_unit(M, nnz)) >= 2048) return 1;
  return std::min<int64_t>(F / 256, 8);
}

int64_t default_unit(int64_t M, int64_t nnz, int64_t F) {
  // Units are equal-sized (S nonzeros), which balances power-law rows by construction.
  // Measured on the Reddit LADIES layers (scripts/spmm_microbench.py, with L2 column
  // tiles): S = 256 is the sweet spot between per-row flush/search overhead (small S) and
  // too few waves per column-tile pass (large S: layer-1 forward 262 us at S = 404 vs
  // 208 us at 256). Small problems keep >= 2048 units for parallelism, S >= 16. Operands
  // with < 16 nonzeros per row on average are mostly output rows to write (the layer-2
  // backward: 8.7 k rows, 1.7 nonzeros each): about two rows per unit, S >= 4 (18 vs 23 us).
  // About 2.4 rows per unit, as a power of two in [16, 256]: the layer-1 backward operand
  // (54 nonzeros per row) 199 us at S = 128 vs 209 at 256; the forward operands (98-114 per
  // row) keep 256.
  int64_t s = row_unit(M, nnz);
  const int64_t t = small_tiles(M, nnz, F);
  if (ceil_div(nnz, s) * t < 2048) s = ceil_div(nnz * t, 2048);
  if (s < 16) s = 16;
  if (M > 0 && nnz < 16 * M) {
    const int64_t r = 2 * nnz / M;
    s = std::min<int64_t>(s, r < 4 ? 4 : r);
  }
  return s;
}

// x16: X rows are 16-bit (gnn_spmm_csr_h16_f32). The call has checked that 4 elements per load
// fit, and everything below is then what the fp32 call picks at VW 4 for this (M, K, nnz, F): the
// summation order of an output depends on G, the unit size and the row kernel's WPR, so equal
// geometry makes the two calls bit-identical on equal values. The L2 tile rule stays in fp32
// columns: a tile's slice of 16-bit X is half the bytes.
SpmmCfg make_cfg(int64_t M, int64_t K, int64_t nnz, int64_t F, int64_t ldx, int64_t ldy, const void* X,
                 const void* Y, int64_t unit, bool x16 = false) {
  SpmmCfg c{};
  c.vw = x16 ? 4 : pick_vw(F, ldx, ldy, X, Y);
  double best = -1.0;
  const int gs[3] = {64, 32, 16};
  for (int gi = 0; gi < 3; ++gi) {
    const int g = gs[gi];
    const int64_t lanecols = (int64_t)c.vw * g;
    const int64_t tiles = ceil_div(F, lanecols * 8) > 0 ? ceil_div(F, lanecols * 8) : 1;
    int64_t nj = ceil_div(F, lanecols * tiles);
    if (nj < 1) nj = 1;
    const double util = (double)F / (double)(tiles * lanecols * nj);
    if (util > best + 1e-9) {
      best = util;
      c.g = g;
      c.nj = (int)nj;
      c.tiles = (int)tiles;
    }
  }
  // L2-sized column tiles. Each XCD's 4 MiB L2 sees random rows of X; when X rows are
  // re-read many times (nnz/K >= 8) cut the columns into tiles whose slice of X
  // (K rows x tile width) is about one L2, processed tile after tile (grid.y is the slow
  // dispatch dimension), so re-reads hit L2 instead of the Infinity Cache. Measured on the
  // Reddit LADIES layers: 1.3-1.9x.
  if (K > 0 && nnz >= 8 * K) {
    const double target_cols = (4.0 * 1024 * 1024 / 4.0) / (double)K;  // floats per row slice
    int64_t cols = (int64_t)c.vw * 16;                                    // smallest: G=16, NJ=1
    while (cols * 2 <= F && (double)(cols * 2) <= target_cols * 1.41421356) cols *= 2;
    if (cols < F) {
      const int64_t per = cols / c.vw;  // lanes x chunks
      c.g = per >= 64 ? 64 : (int)per;
      c.nj = per >= 64 ? (int)(per / 64) : 1;
      if (c.nj > 8) c.nj = 8;
      c.tiles = (int)ceil_div(F, (int64_t)c.vw * c.g * c.nj);
    }
  }
  // Small operands: 256-float column tiles (G = 64, one chunk) for parallelism (small_tiles).
  c.u16 = false;
  if (c.vw == 4 && c.tiles == 1) {
    const int64_t t = small_tiles(M, nnz, F);
    if (t > 1) {
      c.g = 64;
      c.nj = 1;
      c.tiles = (int)ceil_div(F, (int64_t)256);
      const char* e = getenv("GNN_SPMM_SMALL_U16");  // A/B
      c.u16 = !(e && atoi(e) == 0);
    }
  }
  // Experiment override (benchmarks only): GNN_SPMM_G / GNN_SPMM_NJ force the lane group
  // and column chunks; F is then covered by ceil(F / (VW*G*NJ)) column tiles (grid.y).
  if (const char* eg = getenv("GNN_SPMM_G")) {
    const int g = atoi(eg);
    const char* en = getenv("GNN_SPMM_NJ");
    const int nj = en ? atoi(en) : 1;
    const char* ev = getenv("GNN_SPMM_VW");
    if (!x16 && ev && atoi(ev) >= 1 && atoi(ev) < c.vw && (atoi(ev) & (atoi(ev) - 1)) == 0) c.vw = atoi(ev);
    if ((g == 8 || g == 16 || g == 32 || g == 64) && nj >= 1 && nj <= 8) {
      c.g = g;
      c.nj = nj;
      c.tiles = (int)ceil_div(F, (int64_t)c.vw * g * nj);
    }
  }
  c.unit = unit > 0 ? unit : default_unit(M, nnz, F);
  c.nunits = nnz > 0 ? ceil_div(nnz, c.unit) : 1;
  c.ldslab = (int64_t)align_up((size_t)(F > 0 ? F : 1), 4);
  pick_row_kernel(c, M, nnz, F, unit);
  return c;
}

// The XCD map pays when a column tile's slice of X is re-read (several tiles, many units);
// GNN_SPMM_XCD=0/1 forces it off/on (measurements).
WorkMap work_map(const SpmmCfg& c, int64_t M) {
  WorkMap wm{};
  wm.gx = (int)ceil_div(c.nunits + ceil_div(M, (int64_t)ROW_UNIT), 4);
  wm.items = wm.gx * c.tiles;
  bool on = c.tiles > 1;
  if (const char* e = getenv("GNN_SPMM_XCD")) on = atoi(e) != 0;
  wm.xcd_chunk = on ? (int)ceil_div(wm.items, 8) : 0;
  return wm;
}

using MainFn = void (*)(const int*, const int*, const float*, int, int, int, int, const float*, int64_t,
                        float*, int64_t, float*, int64_t, int, const float*, int64_t, const int*, WorkMap);

#ifndef GNN_SPMM_U1  // nonzeros in flight per lane group for one column chunk (experiments: -DGNN_SPMM_U1=n)
#define GNN_SPMM_U1 4
#endif
constexpr int pick_u(int nj) { return nj <= 1 ? GNN_SPMM_U1 : (nj <= 4 ? 4 : (nj == 5 ? 3 : 2)); }

// The kernels of NJ = 1..8 column chunks per lane as a table (I = NJ - 1), without / with residual.
using NJs = std::make_integer_sequence<int, 8>;

template <int VW, int G, int... I>
MainFn main_by_nj(int nj, bool res, std::integer_sequence<int, I...>) {
  static const MainFn t[][2] = {{&spmm_unit_kernel<VW, G, I + 1, pick_u(I + 1), false>,
                                 &spmm_unit_kernel<VW, G, I + 1, pick_u(I + 1), true>}...};
  return nj >= 1 && nj <= 8 ? t[nj - 1][res] : nullptr;
}

template <int VW>
MainFn main_by_g(int g, int nj, bool res) {
  switch (g) {
    case 64: return main_by_nj<VW, 64>(nj, res, NJs{});
    case 32: return main_by_nj<VW, 32>(nj, res, NJs{});
    case 16: return main_by_nj<VW, 16>(nj, res, NJs{});
    case 8: return main_by_nj<VW, 8>(nj, res, NJs{});
    default: return nullptr;
  }
}

// res: the row-mapped residual variant (gnn_spmm_csr_f32_ex); a separate instantiation, so
// the plain aggregation carries no residual code and the two show up apart in rocprofv3.
MainFn select_main(const SpmmCfg& c, bool res) {
  if (c.u16 && c.vw == 4 && c.g == 64 && c.nj == 1)
    return res ? &spmm_unit_kernel<4, 64, 1, 16, true> : &spmm_unit_kernel<4, 64, 1, 16, false>;
  switch (c.vw) {
    case 4: return main_by_g<4>(c.g, c.nj, res);
    case 2: return main_by_g<2>(c.g, c.nj, res);
    case 1: return main_by_g<1>(c.g, c.nj, res);
    default: return nullptr;
  }
}

using RowFn = void (*)(const int*, const int*, const float*, int, const float*, int64_t, float*, int64_t, int, int,
                      const float*, int64_t, const int*);

template <int VW, int NJ, int U>
RowFn row_by_wpr(int wpr, bool res) {
  switch (wpr) {
    case 1: return res ? &spmm_row_kernel<VW, NJ, U, 1, true> : &spmm_row_kernel<VW, NJ, U, 1, false>;
    case 2: return res ? &spmm_row_kernel<VW, NJ, U, 2, true> : &spmm_row_kernel<VW, NJ, U, 2, false>;
    case 4: return res ? &spmm_row_kernel<VW, NJ, U, 4, true> : &spmm_row_kernel<VW, NJ, U, 4, false>;
    case 8: return res ? &spmm_row_kernel<VW, NJ, U, 8, true> : &spmm_row_kernel<VW, NJ, U, 8, false>;
    default: return nullptr;
  }
}

RowFn select_row(const SpmmCfg& c, bool res) {
  if (c.vw == 4) {
    if (c.rnj == 4) return row_by_wpr<4, 4, 4>(c.wpr, res);
    if (c.rnj == 2) return row_by_wpr<4, 2, 8>(c.wpr, res);
    return row_by_wpr<4, 1, 16>(c.wpr, res);
  }
  if (c.rnj != 1) return nullptr;
  if (c.vw == 2) return row_by_wpr<2, 1, 16>(c.wpr, res);
  return row_by_wpr<1, 1, 16>(c.wpr, res);
}

// 16-bit X: VW 4, no residual, G 64 / 32 / 16 (what make_cfg picks without the GNN_SPMM_G override).
using Main16Fn = void (*)(const int*, const int*, const float*, int, int, int, int, const unsigned short*, int64_t,
                          float*, int64_t, float*, int64_t, int, WorkMap);

template <int KIND, int G, int... I>
Main16Fn main16_by_nj(int nj, std::integer_sequence<int, I...>) {
  static const Main16Fn t[] = {&spmm_unit16_kernel<KIND, G, I + 1, pick_u(I + 1)>...};
  return nj >= 1 && nj <= 8 ? t[nj - 1] : nullptr;
}

template <int KIND>
Main16Fn select_main16(const SpmmCfg& c) {
  if (c.u16 && c.g == 64 && c.nj == 1) return &spmm_unit16_kernel<KIND, 64, 1, 16>;
  switch (c.g) {
    case 64: return main16_by_nj<KIND, 64>(c.nj, NJs{});
    case 32: return main16_by_nj<KIND, 32>(c.nj, NJs{});
    case 16: return main16_by_nj<KIND, 16>(c.nj, NJs{});
    default: return nullptr;
  }
}

using Row16Fn = void (*)(const int*, const int*, const float*, int, const unsigned short*, int64_t, float*, int64_t,
                         int, int);

template <int KIND, int NJ, int U>
Row16Fn row16_by_wpr(int wpr) {
  switch (wpr) {
    case 1: return &spmm_row16_kernel<KIND, NJ, U, 1>;
    case 2: return &spmm_row16_kernel<KIND, NJ, U, 2>;
    case 4: return &spmm_row16_kernel<KIND, NJ, U, 4>;
    case 8: return &spmm_row16_kernel<KIND, NJ, U, 8>;
    default: return nullptr;
  }
}

template <int KIND>
Row16Fn select_row16(const SpmmCfg& c) {
  if (c.rnj == 4) return row16_by_wpr<KIND, 4, 4>(c.wpr);
  if (c.rnj == 2) return row16_by_wpr<KIND, 2, 8>(c.wpr);
  return row16_by_wpr<KIND, 1, 16>(c.wpr);
}

// The main kernel's name as rocprofv3 lists it (bench.py's per-kernel roofline).
std::string main_kernel_name(const SpmmCfg& c, bool res) {
  char b[96];
  if (c.wpr)
    snprintf(b, sizeof b, "spmm_row_kernel<%d, %d, %d, %d, %s>", c.vw, c.rnj, c.ru, c.wpr, res ? "true" : "false");
  else
    snprintf(b, sizeof b, "spmm_unit_kernel<%d, %d, %d, %d, %s>", c.vw, c.g, c.nj,
             (c.u16 && c.vw == 4 && c.g == 64 && c.nj == 1) ? 16 : pick_u(c.nj), res ? "true" : "false");
  return b;
}

// The timing hook (gnn_spmm_set_timing_events): a pair of events for this thread's next
// aggregation launch. Every entry point takes it before its first check, so a refused call
// clears it.
thread_local hipEvent_t g_ev_start = nullptr;
thread_local hipEvent_t g_ev_stop = nullptr;

// The one launch of an aggregation kernel. Armed events take the dispatch's own start / end
// timestamps (hipExtLaunchKernel), the kernel's duration as rocprofv3 reports it — not an event
// pair around the launch, which also brackets the queue's event packets (~7 us each).
template <class Fn, class... Args>
void launch_timed(Fn fn, dim3 grid, dim3 block, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, Args... args) {
  if (ev0 || ev1)
    hipExtLaunchKernelGGL(fn, grid, block, 0, st, ev0, ev1, 0, args...);
  else
    hipLaunchKernelGGL(fn, grid, block, 0, st, args...);
}

int check_sizes(const char* nm, int64_t M, int64_t K, int64_t nnz, int64_t F) {
  GNN_REQUIRE(M >= 0 && K >= 0 && nnz >= 0 && F >= 0, "%s: negative size", nm);
  GNN_REQUIRE(M < INT_MAX && K < INT_MAX && nnz < INT_MAX, "%s: M, K, nnz must be < 2^31", nm);
  return 0;
}

constexpr char RES_ALIGN_MSG[] = "gnn_spmm_csr_f32_ex: R (ldr %lld) not aligned for %d-wide vectors";

// The host path of both aggregation calls (nm: the entry point, for the messages) after its own
// checks: early return, NULL checks, configuration, the kernel (sel_row / sel_unit look it up in the
// entry point's tables), its launch and, for the unit kernel, the workspace, overflow and grid checks
// and the combine. `res`: the fp32 kernels' residual arguments (R, ldr, rmap); none for 16-bit X.
template <class XT, class SelRow, class SelUnit, class... Res>
int run_spmm(const char* nm, hipEvent_t ev0, hipEvent_t ev1, const int32_t* rowptr, const int32_t* col,
             const float* val, int64_t M, int64_t K, int64_t nnz, const XT* X, int64_t ldx, float* Y, int64_t ldy,
             int64_t F, const float* R, int64_t ldr, const int32_t* rmap, void* workspace, size_t workspace_bytes,
             int64_t unit_nnz, hipStream_t st, SelRow sel_row, SelUnit sel_unit, Res... res) {
  constexpr bool x16 = sizeof(XT) == 2;
  if (M == 0 || F == 0) return 0;
  GNN_REQUIRE(rowptr && Y, "%s: NULL rowptr/Y", nm);
  GNN_REQUIRE(nnz == 0 || (col && val && X), "%s: NULL col/val/X", nm);
  GNN_REQUIRE(rmap == nullptr || (R != nullptr && F <= ldr), "gnn_spmm_csr_f32_ex: rmap needs R with F <= ldr");
  const SpmmCfg c = make_cfg(M, K, nnz, F, ldx, ldy, X, Y, unit_nnz, x16);
  const bool res_aligned = rmap == nullptr || (ldr % c.vw == 0 && (uintptr_t)R % (4 * c.vw) == 0);
  if (c.wpr) {  // small operand: one workgroup per (row, column slice), nothing to combine
    GNN_REQUIRE(res_aligned, RES_ALIGN_MSG, (long long)ldr, c.vw);
    const auto fn = sel_row(c);
    GNN_REQUIRE(fn != nullptr, "%s: no row kernel for vw=%d nj=%d wpr=%d", nm, c.vw, c.rnj, c.wpr);
    launch_timed(fn, dim3((unsigned)(M * c.slices)), dim3(64 * c.wpr), st, ev0, ev1, rowptr, col, val, (int)M, X, ldx,
                 Y, ldy, (int)F, c.slices, res...);
    GNN_LAUNCHED(x16 ? "spmm_row16_kernel" : "spmm_row_kernel");
    return 0;
  }
  GNN_REQUIRE(c.nunits * c.unit < (int64_t)INT_MAX + c.unit, "%s: unit overflow", nm);
  GNN_REQUIRE(c.nunits <= (int64_t)INT_MAX / 2, "%s: too many units", nm);
  const size_t need = align_up((size_t)c.nunits * 2 * (size_t)c.ldslab * sizeof(float), 256);
  const bool any_split = c.nunits > 1;
  GNN_REQUIRE(!any_split || (workspace && workspace_bytes >= need), "%s: workspace too small (%zu < %zu)", nm,
              workspace_bytes, need);
  GNN_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace not 16-byte aligned", nm);
  GNN_REQUIRE(res_aligned, RES_ALIGN_MSG, (long long)ldr, c.vw);
  const auto fn = sel_unit(c);
  GNN_REQUIRE(fn != nullptr, "%s: no kernel for vw=%d g=%d nj=%d", nm, c.vw, c.g, c.nj);
  float* slab = (float*)workspace;
  GNN_REQUIRE(ceil_div(c.nunits + ceil_div(M, (int64_t)ROW_UNIT), 4) * c.tiles < (int64_t)INT_MAX - 8,
              "%s: grid too large", nm);
  const WorkMap wm = work_map(c, M);
  const dim3 grid((unsigned)(wm.xcd_chunk ? 8 * (int64_t)wm.xcd_chunk : wm.items));
  launch_timed(fn, grid, dim3(256), st, ev0, ev1, rowptr, col, val, (int)M, (int)nnz, (int)c.unit, (int)c.nunits, X,
               ldx, Y, ldy, slab, c.ldslab, (int)F, res..., wm);
  GNN_LAUNCHED(x16 ? "spmm_unit16_kernel" : "spmm_unit_kernel");
  if (any_split) {  // the slab and Y are fp32 whatever X is
    int crows = combine_rows(M);
    if (const char* e = getenv("GNN_SPMM_CROWS")) crows = std::min(64, std::max(1, atoi(e)));  // A/B
    const dim3 g2((unsigned)ceil_div(M, (int64_t)crows));
    auto combine = [&](auto kern) {
      kern<<<g2, dim3(256), 0, st>>>(rowptr, (int)M, (int)c.unit, slab, c.ldslab, Y, ldy, (int)F, R, ldr,
                                     (const int*)rmap, crows);
    };
    // (round 5: for the layer-2 forward, every piece of a pass in flight and a row per workgroup
    // measured equal under the bench — 573.5 / 570.8 vs 574.0 / 570.7 gpu_step: not kept)
    if (c.vw == 4) combine(spmm_combine_kernel<4, COMBINE_LOADS>);
    else if (c.vw == 2) combine(spmm_combine_kernel<2, COMBINE_LOADS>);
    else combine(spmm_combine_kernel<1, COMBINE_LOADS>);
    GNN_LAUNCHED("spmm_combine_kernel");
  }
  return 0;
}

// What gnn_spmm_graph_f32 and gnn_spmm_rows_f32 (nm) check alike, in their order. The timing hook is
// taken first: it belongs to the aggregation launched at the end, and a refused call clears it, as
// the aggregation entry points do. Then the kind, the entry point's own size checks, the strides,
// what gnn_spmm_csr_h16_f32 would refuse (before the block kernel's launch), and the workspace.
template <class SizeChecks>
int block_prologue(const char* nm, hipEvent_t& ev0, hipEvent_t& ev1, int kind, SizeChecks own_size_checks,
                   const void* X, long long ldx, const float* Y, long long ldy, long long F, const void* workspace,
                   size_t workspace_bytes, size_t (*need_bytes)(int64_t, int64_t, int64_t), int64_t rows, int64_t nnz) {
  ev0 = g_ev_start, ev1 = g_ev_stop;
  g_ev_start = g_ev_stop = nullptr;
  GNN_REQUIRE(kind == GNN_FEAT_F32 || kind == GNN_FEAT_F16 || kind == GNN_FEAT_BF16,
              "%s: kind %d is none of GNN_FEAT_F32 (0), GNN_FEAT_F16 (1), GNN_FEAT_BF16 (2)", nm, kind);
  if (const int rc = own_size_checks()) return rc;
  GNN_REQUIRE(F <= ldx, "%s: F (%lld) > ldx (%lld)", nm, F, ldx);
  GNN_REQUIRE(F <= ldy, "%s: F (%lld) > ldy (%lld)", nm, F, ldy);
  if (kind != GNN_FEAT_F32) {
    GNN_REQUIRE(F % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0,
                "%s: 16-bit X: F (%lld), ldx (%lld) and ldy (%lld) must be multiples of 4", nm, F, ldx, ldy);
    GNN_REQUIRE((uintptr_t)X % 8 == 0, "%s: 16-bit X not 8-byte aligned", nm);
    GNN_REQUIRE((uintptr_t)Y % 16 == 0, "%s: 16-bit X: Y not 16-byte aligned", nm);
  }
  const size_t need = need_bytes(rows, nnz, F);
  GNN_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", nm,
              workspace ? workspace_bytes : (size_t)0, need);
  GNN_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace not 16-byte aligned", nm);
  return 0;
}

// Their common end: the hook handed on, past the block kernel's launch, to the aggregation over
// the block-local CSR, with the workspace from `ws` on as its slab.
int block_aggregate(hipEvent_t ev0, hipEvent_t ev1, const int32_t* rowptr, const int32_t* col, const float* val,
                    int64_t M, int64_t K, int64_t nnz, const void* X, int64_t ldx, int kind, float* Y, int64_t ldy,
                    int64_t F, void* workspace, size_t workspace_bytes, char* ws, hipStream_t st) {
  const size_t rest = workspace_bytes - (size_t)(ws - (char*)workspace);
  g_ev_start = ev0;
  g_ev_stop = ev1;
  if (kind == GNN_FEAT_F32)
    return gnn_spmm_csr_f32(rowptr, col, val, M, K, nnz, (const float*)X, ldx, Y, ldy, F, ws, rest, 0, st);
  return gnn_spmm_csr_h16_f32(rowptr, col, val, M, K, nnz, X, ldx, kind, Y, ldy, F, ws, rest, 0, st);
}

// The workspace of a block call: the row pointer, the weights, with `own_cols` the relabelled
// columns, and the aggregation's share. That is gnn_spmm_workspace_bytes(rows, nnz, F, 0) raised to
// a bound that grows with rows and nnz, so one workspace sized for the largest block of a plan
// serves every smaller one. default_unit's unit count itself is not monotone (the unit size doubles
// as rows get longer); it never exceeds max(2048, min(nnz / 4, 1.25 rows) + nnz / 256) (units of
// >= 256 entries for long rows, about two rows or >= 4 entries per unit for short ones). With
// own_cols (gnn_spmm_rows_f32) the bound is cut at nnz / 4 + 1 (a unit never holds fewer than 4
// entries: default_unit), itself monotone — so the few-row blocks of a small closure do not pay the
// 2,048-unit floor.
size_t block_workspace_bytes(int64_t rows, int64_t nnz, int64_t F, bool own_cols) {
  const int64_t r = rows > 0 ? rows : 0, n = nnz > 0 ? nnz : 0;
  int64_t units = std::max<int64_t>(2048, std::min(ceil_div(n, 4), r + r / 4 + 2) + ceil_div(n, 256) + 1);
  if (own_cols) units = std::min(units, ceil_div(n, 4) + 1);
  const size_t slab = align_up((size_t)(F > 0 ? F : 1), 4) * 2 * sizeof(float);
  const size_t agg = std::max(align_up((size_t)units * slab, 256), gnn_spmm_workspace_bytes(r, n, F, 0));
  return align_up(((size_t)r + 1) * sizeof(int32_t), 256) + (own_cols ? 2 : 1) * align_up((size_t)n * sizeof(float), 256) +
         agg;
}

void fill_config(const SpmmCfg& c, int32_t* out) {
  const int32_t v[6] = {c.vw, c.g, c.nj, c.tiles, (int32_t)c.unit, (int32_t)c.nunits};
  std::copy(v, v + 6, out);
}

}  // namespace

bool gnn::spmm_row_chain(int64_t M, int64_t K, int64_t nnz, int64_t F, int64_t ldx, int64_t ldy, const void* X,
                         const void* Y) {
  const SpmmCfg c = make_cfg(M, K, nnz, F, ldx, ldy, X, Y, 0);
  return c.wpr == 1 && c.vw == 4;
}

extern "C" {

int64_t gnn_spmm_default_unit_nnz(int64_t M, int64_t nnz, int64_t F) { return default_unit(M, nnz, F); }

size_t gnn_spmm_workspace_bytes(int64_t M, int64_t nnz, int64_t F, int64_t unit_nnz) {
  const SpmmCfg c = make_cfg(M, 0, nnz, F, F, F, nullptr, nullptr, unit_nnz);
  // (the row kernel needs none; the size stays the unit kernel's, which a call with other
  // strides / alignment may take)
  return align_up((size_t)c.nunits * 2 * (size_t)c.ldslab * sizeof(float), 256);
}

int gnn_spmm_kernel_name(int64_t M, int64_t K, int64_t nnz, int64_t F, int64_t ldx, int64_t ldy, const void* X,
                         const void* Y, int64_t unit_nnz, int residual, char* out, size_t out_bytes) {
  GNN_REQUIRE(out != nullptr && out_bytes > 0, "gnn_spmm_kernel_name: out is NULL");
  const std::string n = main_kernel_name(make_cfg(M, K, nnz, F, ldx, ldy, X, Y, unit_nnz), residual != 0);
  snprintf(out, out_bytes, "%s", n.c_str());
  return 0;
}

int gnn_spmm_config(int64_t M, int64_t K, int64_t nnz, int64_t F, int64_t ldx, int64_t ldy, const void* X,
                    const void* Y, int64_t unit_nnz, int32_t out[6]) {
  GNN_REQUIRE(out != nullptr, "gnn_spmm_config: out is NULL");
  fill_config(make_cfg(M, K, nnz, F, ldx, ldy, X, Y, unit_nnz), out);
  return 0;
}

int gnn_spmm_h16_config(int64_t M, int64_t K, int64_t nnz, int64_t F, int64_t ldx, int64_t ldy, const void* X,
                        const void* Y, int64_t unit_nnz, int32_t out[8]) {
  GNN_REQUIRE(out != nullptr, "gnn_spmm_h16_config: out is NULL");
  const SpmmCfg c = make_cfg(M, K, nnz, F, ldx, ldy, X, Y, unit_nnz, true);
  fill_config(c, out);
  out[6] = c.wpr;
  out[7] = 4;  // 16-bit elements per load
  return 0;
}

void gnn_spmm_set_timing_events(void* start, void* stop) {
  g_ev_start = (hipEvent_t)start;
  g_ev_stop = (hipEvent_t)stop;
}

int gnn_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t M, int64_t K,
                     int64_t nnz, const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t F,
                     void* workspace, size_t workspace_bytes, int64_t unit_nnz, void* stream) {
  return gnn_spmm_csr_f32_ex(rowptr, col, val, M, K, nnz, X, ldx, Y, ldy, F, nullptr, 0, nullptr, workspace,
                             workspace_bytes, unit_nnz, stream);
}

int gnn_spmm_csr_f32_ex(const int32_t* rowptr, const int32_t* col, const float* val, int64_t M, int64_t K,
                        int64_t nnz, const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t F,
                        const float* R, int64_t ldr, const int32_t* rmap, void* workspace, size_t workspace_bytes,
                        int64_t unit_nnz, void* stream) {
  hipEvent_t ev0 = g_ev_start, ev1 = g_ev_stop;
  g_ev_start = g_ev_stop = nullptr;
  if (const int rc = check_sizes("gnn_spmm_csr_f32", M, K, nnz, F)) return rc;
  GNN_REQUIRE(F <= ldx || K == 0, "gnn_spmm_csr_f32: F (%lld) > ldx (%lld)", (long long)F, (long long)ldx);
  GNN_REQUIRE(F <= ldy || M == 0, "gnn_spmm_csr_f32: F (%lld) > ldy (%lld)", (long long)F, (long long)ldy);
  const bool res = rmap != nullptr;  // (R's alignment: checked against the vector width run_spmm picks)
  return run_spmm(
      "gnn_spmm_csr_f32", ev0, ev1, rowptr, col, val, M, K, nnz, X, ldx, Y, ldy, F, R, ldr, rmap, workspace,
      workspace_bytes, unit_nnz, (hipStream_t)stream, [&](const SpmmCfg& c) { return select_row(c, res); },
      [&](const SpmmCfg& c) { return select_main(c, res); }, R, ldr, (const int*)rmap);
}

int gnn_spmm_csr_h16_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t M, int64_t K,
                         int64_t nnz, const void* X, int64_t ldx, int kind, float* Y, int64_t ldy, int64_t F,
                         void* workspace, size_t workspace_bytes, int64_t unit_nnz, void* stream) {
  hipEvent_t ev0 = g_ev_start, ev1 = g_ev_stop;
  g_ev_start = g_ev_stop = nullptr;
  GNN_REQUIRE(kind == GNN_FEAT_F16 || kind == GNN_FEAT_BF16,
              "gnn_spmm_csr_h16_f32: kind %d is neither GNN_FEAT_F16 (1) nor GNN_FEAT_BF16 (2)", kind);
  if (const int rc = check_sizes("gnn_spmm_csr_h16_f32", M, K, nnz, F)) return rc;
  GNN_REQUIRE(F <= ldx, "gnn_spmm_csr_h16_f32: F (%lld) > ldx (%lld)", (long long)F, (long long)ldx);
  GNN_REQUIRE(F <= ldy, "gnn_spmm_csr_h16_f32: F (%lld) > ldy (%lld)", (long long)F, (long long)ldy);
  // 4 elements per load and no scalar form: callers whose rows do not fit widen first
  GNN_REQUIRE(F % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0,
              "gnn_spmm_csr_h16_f32: F (%lld), ldx (%lld) and ldy (%lld) must be multiples of 4", (long long)F,
              (long long)ldx, (long long)ldy);
  GNN_REQUIRE((uintptr_t)X % 8 == 0, "gnn_spmm_csr_h16_f32: X not 8-byte aligned");
  GNN_REQUIRE((uintptr_t)Y % 16 == 0, "gnn_spmm_csr_h16_f32: Y not 16-byte aligned");
  const bool f16 = kind == GNN_FEAT_F16;
  return run_spmm(
      "gnn_spmm_csr_h16_f32", ev0, ev1, rowptr, col, val, M, K, nnz, (const unsigned short*)X, ldx, Y, ldy, F, nullptr,
      0, nullptr, workspace, workspace_bytes, unit_nnz, (hipStream_t)stream,
      [&](const SpmmCfg& c) { return f16 ? select_row16<GNN_FEAT_F16>(c) : select_row16<GNN_FEAT_BF16>(c); },
      [&](const SpmmCfg& c) { return f16 ? select_main16<GNN_FEAT_F16>(c) : select_main16<GNN_FEAT_BF16>(c); });
}

size_t gnn_spmm_graph_workspace_bytes(int64_t rows, int64_t nnz, int64_t F) {
  return block_workspace_bytes(rows, nnz, F, false);
}

int gnn_spmm_graph_f32(const int64_t* indptr, const int32_t* indices, const int32_t* degree, int64_t num_nodes,
                       int64_t row0, int64_t rows, int64_t e0, int64_t nnz, const void* X, int64_t ldx, int kind,
                       float* Y, int64_t ldy, int64_t F, void* workspace, size_t workspace_bytes, void* stream) {
  hipEvent_t ev0, ev1;
  auto own_size_checks = [&] {
    GNN_REQUIRE(num_nodes >= 0 && row0 >= 0 && rows >= 0 && e0 >= 0 && nnz >= 0 && F >= 0,
                "gnn_spmm_graph_f32: negative size (num_nodes, row0, rows, e0, nnz or F)");
    GNN_REQUIRE(rows < INT_MAX && nnz < INT_MAX && num_nodes < INT_MAX,
                "gnn_spmm_graph_f32: rows, nnz and num_nodes must be < 2^31");
    GNN_REQUIRE(row0 <= num_nodes && rows <= num_nodes - row0,
                "gnn_spmm_graph_f32: row0 (%lld) + rows (%lld) > num_nodes (%lld)", (long long)row0, (long long)rows,
                (long long)num_nodes);
    return 0;
  };
  const int rc = block_prologue("gnn_spmm_graph_f32", ev0, ev1, kind, own_size_checks, X, ldx, Y, ldy, F, workspace,
                                workspace_bytes, gnn_spmm_graph_workspace_bytes, rows, nnz);
  if (rc || rows == 0 || F == 0) return rc;
  GNN_REQUIRE(indptr && degree && Y, "gnn_spmm_graph_f32: NULL indptr/degree/Y");
  GNN_REQUIRE(nnz == 0 || (indices && X), "gnn_spmm_graph_f32: NULL indices/X");
  char* ws = (char*)workspace;
  int32_t* rowptr = (int32_t*)ws;
  ws += align_up(((size_t)rows + 1) * sizeof(int32_t), 256);
  float* val = (float*)ws;
  ws += align_up((size_t)nnz * sizeof(float), 256);
  hipStream_t st = (hipStream_t)stream;
  graph_block_kernel<<<dim3((unsigned)ceil_div(rows + 1, 4)), dim3(256), 0, st>>>(indptr, degree, row0, (int)rows, e0,
                                                                                 (int)nnz, rowptr, val);
  GNN_LAUNCHED("graph_block_kernel");
  // the block's columns are the graph's own, read in place: the aggregation loads col per lane
  return block_aggregate(ev0, ev1, rowptr, indices ? indices + e0 : nullptr, val, rows, num_nodes, nnz, X, ldx, kind,
                         Y, ldy, F, workspace, workspace_bytes, ws, st);
}

size_t gnn_spmm_rows_workspace_bytes(int64_t rows, int64_t nnz, int64_t F) {
  return block_workspace_bytes(rows, nnz, F, true);
}

int gnn_spmm_rows_f32(const int64_t* indptr, const int32_t* indices, const int32_t* degree, int64_t num_nodes,
                      const int32_t* rows, int64_t M, const int32_t* rowseg, int64_t nnz, const void* table, int64_t K,
                      const void* X, int64_t ldx, int kind, float* Y, int64_t ldy, int64_t F, void* workspace,
                      size_t workspace_bytes, int32_t* err_flag, void* stream) {
  hipEvent_t ev0, ev1;
  auto own_size_checks = [&] {
    GNN_REQUIRE(num_nodes >= 0 && M >= 0 && nnz >= 0 && K >= 0 && F >= 0,
                "gnn_spmm_rows_f32: negative size (num_nodes, M, nnz, K or F)");
    GNN_REQUIRE(M < INT_MAX && nnz < INT_MAX && num_nodes < INT_MAX && K < INT_MAX,
                "gnn_spmm_rows_f32: M, nnz, num_nodes and K must be < 2^31");
    GNN_REQUIRE(K <= num_nodes, "gnn_spmm_rows_f32: K (%lld) > num_nodes (%lld)", (long long)K, (long long)num_nodes);
    return 0;
  };
  const int rc = block_prologue("gnn_spmm_rows_f32", ev0, ev1, kind, own_size_checks, X, ldx, Y, ldy, F, workspace,
                                workspace_bytes, gnn_spmm_rows_workspace_bytes, M, nnz);
  if (rc || M == 0 || F == 0) return rc;
  GNN_REQUIRE(indptr && degree && rows && rowseg && Y, "gnn_spmm_rows_f32: NULL indptr/degree/rows/rowseg/Y");
  GNN_REQUIRE(table != nullptr && (uintptr_t)table % 8 == 0, "gnn_spmm_rows_f32: NULL or misaligned table");
  GNN_REQUIRE(nnz == 0 || (indices && X), "gnn_spmm_rows_f32: NULL indices/X");
  char* ws = (char*)workspace;
  int32_t* rowptr = (int32_t*)ws;
  ws += align_up(((size_t)M + 1) * sizeof(int32_t), 256);
  int32_t* col = (int32_t*)ws;
  ws += align_up((size_t)nnz * sizeof(int32_t), 256);
  float* val = (float*)ws;
  ws += align_up((size_t)nnz * sizeof(float), 256);
  hipStream_t st = (hipStream_t)stream;
  rows_block_kernel<<<dim3((unsigned)ceil_div(M + 1, 4)), dim3(256), 0, st>>>(
      indptr, indices, degree, (int)num_nodes, rows, (int)M, rowseg, (int)nnz, (const uint2*)table, (int)K, rowptr, col,
      val, err_flag);
  GNN_LAUNCHED("rows_block_kernel");
  return block_aggregate(ev0, ev1, rowptr, col, val, M, K, nnz, X, ldx, kind, Y, ldy, F, workspace, workspace_bytes, ws,
                         st);
}

}  // extern "C"
