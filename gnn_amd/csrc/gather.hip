// gather.hip — the row gathers that stage features: fp32 rows, 16-bit rows widened to fp32 on the
// way, each from one source or from two in one launch, and fp32 rows read straight from pinned host
// memory, and rows by node id over a placed store (the placement map names each row's source). One
// wave per row, stream-ordered, no allocation. Kernels and the gnn_gather_rows* / gnn_gather_placed*
// C ABI.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <algorithm>

#include "gnn_spmm.h"
#include "common.h"
#include "spmm_device.h"

namespace {

using gnn::ceil_div;
using gnn::pick_vw;

// ---------------------------------------------------------------------------------
// Feature staging gather/scatter: one wave per row.
// ---------------------------------------------------------------------------------
template <int VW>
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, int64_t ld_src,
                                                          const int64_t* __restrict__ src_idx,
                                                          float* __restrict__ dst, int64_t ld_dst,
                                                          const int64_t* __restrict__ dst_idx,
                                                          int64_t n, int F) {
  using V = typename Vec<VW>::T;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t s = src_idx ? src_idx[i] : i;
  const int64_t d = dst_idx ? dst_idx[i] : i;
  const float* sr = src + s * ld_src;
  float* dr = dst + d * ld_dst;
  for (int c = lane * VW; c < F; c += 64 * VW) {
    *reinterpret_cast<V*>(dr + c) = *reinterpret_cast<const V*>(sr + c);
  }
}

// X0 from two sources in one launch (round 6): rows [0, n0) from (src0, idx0) and
// rows [n0, n0 + n1) from (src1, idx1), to dst rows pos0 / pos1 — the own feature-buffer rows and
// the batch's host rows of a staging issue. A wave per row with every load of the row issued
// before its stores (608-float rows: 3 float4 per lane).
template <int VW, int NL>
__global__ __launch_bounds__(256) void gather_rows2_kernel(const float* __restrict__ src0, int64_t ld0,
                                                           const int64_t* __restrict__ idx0,
                                                           const int64_t* __restrict__ pos0, int64_t n0,
                                                           const float* __restrict__ src1, int64_t ld1,
                                                           const int64_t* __restrict__ idx1,
                                                           const int64_t* __restrict__ pos1, int64_t n1,
                                                           float* __restrict__ dst, int64_t ld_dst, int F) {
  using V = typename Vec<VW>::T;
  const int lane = threadIdx.x & 63;
  int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n0 + n1) return;
  const bool second = i >= n0;  // wave-uniform
  if (second) i -= n0;
  const float* sr;
  int64_t d;
  if (!second) {
    sr = src0 + (idx0 ? idx0[i] : i) * ld0;
    d = pos0 ? pos0[i] : i;
  } else {
    sr = src1 + (idx1 ? idx1[i] : i) * ld1;
    d = pos1 ? pos1[i] : i;
  }
  float* dr = dst + d * ld_dst;
  V v[NL];
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const int c = (lane + 64 * k) * VW;
    if (c < F) v[k] = *reinterpret_cast<const V*>(sr + c);
  }
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const int c = (lane + 64 * k) * VW;
    if (c < F) *reinterpret_cast<V*>(dr + c) = v[k];
  }
}

// ---------------------------------------------------------------------------------
// 16-bit feature stores (GNN_FEAT_F16 / GNN_FEAT_BF16): the same gathers, widening to fp32 on the
// way (main.py:132-134's `.float()`). Both conversions are exact, so X0 equals
// feats.float()[input_nodes] bit for bit. A wave per row; a lane loads VW 16-bit elements at a
// time (VW 8: one 16-byte load, two float4 stores), NL loads in flight before the first store
// (a 608-column row: two 16-byte loads per lane).
// ---------------------------------------------------------------------------------
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef unsigned short us4 __attribute__((ext_vector_type(4)));
typedef unsigned short us8 __attribute__((ext_vector_type(8)));
template <int VW> struct Vec16;
template <> struct Vec16<1> { using T = unsigned short; };
template <> struct Vec16<2> { using T = us2; };
template <> struct Vec16<4> { using T = us4; };
template <> struct Vec16<8> { using T = us8; };

// bf16 is the upper half of the fp32 pattern; fp16 is the hardware convert (v_cvt_f32_f16: fp16
// denormals are always on for gfx9 code objects, so subnormals widen exactly; NaN stays NaN).
template <int KIND>
__device__ __forceinline__ float widen16(unsigned short b) {
  if constexpr (KIND == GNN_FEAT_BF16) {
    return __uint_as_float((unsigned)b << 16);
  } else {
    return (float)__builtin_bit_cast(_Float16, b);
  }
}

// Columns [c0, c0 + 64 * VW * NL) of one row, in two halves: every load issued (widen_load), then
// the widened stores (widen_store).
template <int VW, int NL>
__device__ __forceinline__ void widen_load(const unsigned short* __restrict__ sr, int c0, int F, int lane,
                                           typename Vec16<VW>::T (&v)[NL]) {
  using S = typename Vec16<VW>::T;
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const int c = c0 + (lane + 64 * k) * VW;
    if (c < F) v[k] = *reinterpret_cast<const S*>(sr + c);
  }
}

template <int KIND, int VW, int NL>
__device__ __forceinline__ void widen_store(float* __restrict__ dr, int c0, int F, int lane,
                                            const typename Vec16<VW>::T (&v)[NL]) {
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const int c = c0 + (lane + 64 * k) * VW;
    if (c >= F) continue;
    if constexpr (VW == 1) {
      dr[c] = widen16<KIND>(v[k]);
    } else {
      constexpr int OW = VW < 4 ? VW : 4;
      using O = typename Vec<OW>::T;
#pragma unroll
      for (int q = 0; q < VW; q += OW) {
        O o;
#pragma unroll
        for (int j = 0; j < OW; ++j) o[j] = widen16<KIND>(v[k][q + j]);
        *reinterpret_cast<O*>(dr + c + q) = o;
      }
    }
  }
}

template <int KIND, int VW, int NL>
__device__ __forceinline__ void widen_pass(const unsigned short* __restrict__ sr, float* __restrict__ dr, int c0,
                                           int F, int lane) {
  typename Vec16<VW>::T v[NL];
  widen_load<VW, NL>(sr, c0, F, lane, v);
  widen_store<KIND, VW, NL>(dr, c0, F, lane, v);
}

template <int KIND, int VW, int NL>
__global__ __launch_bounds__(256) void gather_rows_h16_kernel(const unsigned short* __restrict__ src, int64_t ld_src,
                                                              const int64_t* __restrict__ src_idx,
                                                              float* __restrict__ dst, int64_t ld_dst,
                                                              const int64_t* __restrict__ dst_idx, int64_t n, int F) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const unsigned short* sr = src + (src_idx ? src_idx[i] : i) * ld_src;
  float* dr = dst + (dst_idx ? dst_idx[i] : i) * ld_dst;
  for (int c0 = 0; c0 < F; c0 += 64 * VW * NL) widen_pass<KIND, VW, NL>(sr, dr, c0, F, lane);
}

// The two-source form (gather_rows2_kernel): rows of at most 64 * VW * NL columns, one pass.
template <int KIND, int VW, int NL>
__global__ __launch_bounds__(256) void gather_rows2_h16_kernel(const unsigned short* __restrict__ src0, int64_t ld0,
                                                               const int64_t* __restrict__ idx0,
                                                               const int64_t* __restrict__ pos0, int64_t n0,
                                                               const unsigned short* __restrict__ src1, int64_t ld1,
                                                               const int64_t* __restrict__ idx1,
                                                               const int64_t* __restrict__ pos1, int64_t n1,
                                                               float* __restrict__ dst, int64_t ld_dst, int F) {
  const int lane = threadIdx.x & 63;
  int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n0 + n1) return;
  const bool second = i >= n0;  // wave-uniform
  if (second) i -= n0;
  const unsigned short* sr;
  int64_t d;
  if (!second) {
    sr = src0 + (idx0 ? idx0[i] : i) * ld0;
    d = pos0 ? pos0[i] : i;
  } else {
    sr = src1 + (idx1 ? idx1[i] : i) * ld1;
    d = pos1 ? pos1[i] : i;
  }
  widen_pass<KIND, VW, NL>(sr, dst + d * ld_dst, 0, F, lane);
}

// Rows read straight from pinned, device-mapped host memory (zero-copy over PCIe): a small
// persistent grid (each wave two rows per pass, every load of both rows issued before the
// first store) keeps a few MB of PCIe reads in flight while holding few CU slots, so the
// gather runs on the staging stream beside the compute kernels.
// Measured on MI355X (Reddit batch, 31 MB of host rows): 46-51 GB/s at 32-128 workgroups,
// 24 GB/s at 8 — but the PCIe reads slow the concurrent compute kernels (GPU step 2.18 ->
// 2.50-2.64 ms at every grid tried), so bench.py defaults to the pinned-copy path.
constexpr int HOST_GATHER_GRID = 32;

template <int VW>
__global__ __launch_bounds__(256) void gather_rows_host_kernel(const float* __restrict__ src, int64_t ld_src,
                                                               const int64_t* __restrict__ src_idx,
                                                               float* __restrict__ dst, int64_t ld_dst,
                                                               const int64_t* __restrict__ dst_idx, int64_t n, int F) {
  using V = typename Vec<VW>::T;
  constexpr int CH = 3;  // 64 * VW-float chunks per row held in registers (608 floats at VW 4)
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t i0 = 2 * w; i0 < n; i0 += 2 * nw) {
    V v[2][CH];
    const float* sr[2];
    float* dr[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t i = min(i0 + q, n - 1);  // an odd last row is simply copied twice
      sr[q] = src + (src_idx ? src_idx[i] : i) * ld_src;
      dr[q] = dst + (dst_idx ? dst_idx[i] : i) * ld_dst;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int c = (lane + 64 * j) * VW;
        if (c < F) v[q][j] = *reinterpret_cast<const V*>(sr[q] + c);
      }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int c = (lane + 64 * j) * VW;
        if (c < F) *reinterpret_cast<V*>(dr[q] + c) = v[q][j];
      }
      for (int c = (lane + 64 * CH) * VW; c < F; c += 64 * VW)  // rows wider than CH chunks
        *reinterpret_cast<V*>(dr[q] + c) = *reinterpret_cast<const V*>(sr[q] + c);
    }
  }
}

// Elements per load of a 16-bit source row (gather_rows_h16_kernel): 8 (16 bytes) when every row
// of src and dst allows it, else 4, 2 or 1 (any stride >= F and any 2-byte-aligned base works).
int pick_vw16(int64_t F, int64_t ld_src, int64_t ld_dst, const void* src, const void* dst) {
  const uintptr_t ps = (uintptr_t)src, pd = (uintptr_t)dst;
  const bool d4 = ld_dst % 4 == 0 && pd % 16 == 0;
  if (F % 8 == 0 && ld_src % 8 == 0 && ps % 16 == 0 && d4) return 8;
  if (F % 4 == 0 && ld_src % 4 == 0 && ps % 8 == 0 && d4) return 4;
  if (F % 2 == 0 && ld_src % 2 == 0 && ps % 4 == 0 && ld_dst % 2 == 0 && pd % 8 == 0) return 2;
  return 1;
}

// Loads per lane and pass of the 16-bit gathers: 1024 columns at VW 8 / 4, 512 at VW 2 / 1.
constexpr int h16_nl(int vw) { return vw == 8 ? 2 : (vw == 1 ? 8 : 4); }

// ---------------------------------------------------------------------------------
// X0 by node id over a placed feature store (gnn_gather_placed_f32): every position looks its
// node up in the placement map and reads the row from the source the map names — a buffer in
// device memory (this rank's, or a mapped peer's) or the registered host table. One launch, two
// roles chosen by blockIdx: the first `walkers` workgroups are the host walkers, the rest take the
// device rows, a wave per position. Every position is served by exactly one role: the device wave
// of a host-placed node returns, and a walker skips every node that is not host-placed (a node
// outside the map is the device wave's to zero and flag).
// ---------------------------------------------------------------------------------
constexpr int PLACE_SLOT_MASK = (1 << GNN_PLACE_SHIFT) - 1;

// Loads per lane and pass: fp32 rows 768 columns at every width, 16-bit rows as h16_nl.
template <int KIND, int VW>
constexpr int placed_nl() {
  if constexpr (KIND == GNN_FEAT_F32) return 12 / VW;
  else return h16_nl(VW);
}

// One pass of one row held in registers: load() issues every load, store() the (widened) stores.
template <int KIND, int VW>
struct PlacedPass {
  static constexpr int NL = placed_nl<KIND, VW>();
  static constexpr int COLS = 64 * VW * NL;
  using E = unsigned short;
  typename Vec16<VW>::T v[NL];
  __device__ __forceinline__ void load(const E* __restrict__ sr, int c0, int F, int lane) {
    widen_load<VW, NL>(sr, c0, F, lane, v);
  }
  __device__ __forceinline__ void store(float* __restrict__ dr, int c0, int F, int lane) const {
    widen_store<KIND, VW, NL>(dr, c0, F, lane, v);
  }
};

template <int VW>
struct PlacedPass<GNN_FEAT_F32, VW> {
  static constexpr int NL = placed_nl<GNN_FEAT_F32, VW>();
  static constexpr int COLS = 64 * VW * NL;
  using E = float;
  using V = typename Vec<VW>::T;
  V v[NL];
  __device__ __forceinline__ void load(const E* __restrict__ sr, int c0, int F, int lane) {
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int c = c0 + (lane + 64 * k) * VW;
      if (c < F) v[k] = *reinterpret_cast<const V*>(sr + c);
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ dr, int c0, int F, int lane) const {
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int c = c0 + (lane + 64 * k) * VW;
      if (c < F) *reinterpret_cast<V*>(dr + c) = v[k];
    }
  }
};

template <int KIND>
using placed_elem = typename PlacedPass<KIND, 1>::E;

template <int KIND>
__device__ __forceinline__ float placed_widen(placed_elem<KIND> e) {
  if constexpr (KIND == GNN_FEAT_F32) return e;
  else return widen16<KIND>(e);
}

// One row, a wave: every load of a pass before its stores; rows wider than a pass loop. The
// row's whole VW-element vectors move as vectors and the F % VW columns after them one per lane,
// so a 602-column row moves by 16-byte loads without touching the padding behind it.
template <int KIND, int VW>
__device__ __forceinline__ void placed_row(const placed_elem<KIND>* __restrict__ sr, float* __restrict__ dr, int F,
                                           int lane) {
  const int Fv = F - F % VW;
  placed_elem<KIND> t{};
  if (VW > 1 && Fv + lane < F) t = sr[Fv + lane];
  for (int c0 = 0; c0 < Fv; c0 += PlacedPass<KIND, VW>::COLS) {
    PlacedPass<KIND, VW> p;
    p.load(sr, c0, Fv, lane);
    p.store(dr, c0, Fv, lane);
  }
  if (VW > 1 && Fv + lane < F) dr[Fv + lane] = placed_widen<KIND>(t);
}

// Two rows, a wave (the host walkers: twice the PCIe reads in flight per wave).
template <int KIND, int VW>
__device__ __forceinline__ void placed_pair(const placed_elem<KIND>* s0, const placed_elem<KIND>* s1, float* d0,
                                            float* d1, int F, int lane) {  // (an odd last row: s1 == s0, d1 == d0)
  const int Fv = F - F % VW;
  placed_elem<KIND> t0{}, t1{};
  if (VW > 1 && Fv + lane < F) {
    t0 = s0[Fv + lane];
    t1 = s1[Fv + lane];
  }
  for (int c0 = 0; c0 < Fv; c0 += PlacedPass<KIND, VW>::COLS) {
    PlacedPass<KIND, VW> p0, p1;
    p0.load(s0, c0, Fv, lane);
    p1.load(s1, c0, Fv, lane);
    p0.store(d0, c0, Fv, lane);
    p1.store(d1, c0, Fv, lane);
  }
  if (VW > 1 && Fv + lane < F) {
    d0[Fv + lane] = placed_widen<KIND>(t0);
    d1[Fv + lane] = placed_widen<KIND>(t1);
  }
}

// Elements per load of a source's rows: the widest of CAP, CAP / 2, .. 1 that its base and stride
// allow (CAP is what dst allows, the host's choice). Wave-uniform.
template <int KIND, int CAP>
__device__ __forceinline__ int placed_vw(const void* base, int64_t ld) {
  const uint64_t a = (uint64_t)(uintptr_t)base / sizeof(placed_elem<KIND>) | (uint64_t)ld;  // in elements
  int vw = CAP;
  while (vw > 1 && (a & (uint64_t)(vw - 1))) vw >>= 1;
  return vw;
}

__device__ __forceinline__ void placed_zero_row(float* __restrict__ dr, int F, int lane, int32_t* flag) {
  for (int c = lane; c < F; c += 64) dr[c] = 0.f;
  if (lane == 0) atomicOr(flag, 1);
}

template <int KIND, int CAP>
__global__ __launch_bounds__(256) void gather_placed_kernel(const int32_t* __restrict__ place, int num_nodes,
                                                            const gnn_place_src* __restrict__ srcs, int nsrc,
                                                            const void* __restrict__ host_table, int64_t ld_host,
                                                            const int32_t* __restrict__ nodes, int64_t n,
                                                            float* __restrict__ dst, int64_t ld_dst, int F,
                                                            int64_t* __restrict__ counts, int32_t* __restrict__ flag,
                                                            int walkers) {
  using E = placed_elem<KIND>;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if ((int)blockIdx.x >= walkers) {
    // ---- a device row: place -> (source, slot), both wave-uniform (scalar loads) ----
    const int64_t i = (int64_t)(blockIdx.x - walkers) * 4 + wv;
    if (i >= n) return;
    const int node = nodes[i];
    float* dr = dst + i * ld_dst;
    if ((unsigned)node >= (unsigned)num_nodes) return placed_zero_row(dr, F, lane, flag);
    const int p = place[node];
    if (p == GNN_PLACE_HOST) return;  // a walker's row
    const unsigned s = (unsigned)p >> GNN_PLACE_SHIFT;  // a negative value other than -1: >= 16
    if (s >= (unsigned)nsrc) return placed_zero_row(dr, F, lane, flag);
    const void* base = srcs[s].base;
    const int64_t ld = srcs[s].ld, rows = srcs[s].rows;
    const int64_t slot = p & PLACE_SLOT_MASK;
    if (base == nullptr || slot >= rows || ld < F) return placed_zero_row(dr, F, lane, flag);
    const E* sr = (const E*)base + slot * ld;
    const int vw = placed_vw<KIND, CAP>(base, ld);
    if constexpr (CAP >= 8) if (vw == 8) return placed_row<KIND, 8>(sr, dr, F, lane);
    if constexpr (CAP >= 4) if (vw == 4) return placed_row<KIND, 4>(sr, dr, F, lane);
    if constexpr (CAP >= 2) if (vw == 2) return placed_row<KIND, 2>(sr, dr, F, lane);
    return placed_row<KIND, 1>(sr, dr, F, lane);
  }
  // ---- a host walker: a contiguous range of positions per wave, 64 map values at a time; the
  // host-placed ones are balloted and walked two rows at a time. No list, no atomic, no counter:
  // the range is a function of (n, walkers) alone. The same pass tallies `counts` (lane s: the
  // rows source s serves, lane nsrc: the host's), one add per wave at its end.
  const int64_t nw = (int64_t)walkers * 4;
  const int64_t chunk = (n + nw - 1) / nw;
  const int64_t start = ((int64_t)blockIdx.x * 4 + wv) * chunk;
  const int64_t end = start + chunk < n ? start + chunk : n;
  const E* host = (const E*)host_table;
  const int vwh = host ? placed_vw<KIND, CAP>(host, ld_host) : 1;
  int64_t cnt = 0;
  for (int64_t i0 = start; i0 < end; i0 += 64) {
    const int64_t i = i0 + lane;
    const int node = i < end ? nodes[i] : -1;
    const bool valid = (unsigned)node < (unsigned)num_nodes;
    const int p = valid ? place[node] : 0;
    unsigned long long hm = __ballot(valid && p == GNN_PLACE_HOST);
    if (counts) {
      const unsigned s_of = (unsigned)p >> GNN_PLACE_SHIFT;
      const int64_t slot = p & PLACE_SLOT_MASK;
      for (int s = 0; s < nsrc; ++s) {
        const bool live = srcs[s].base != nullptr && srcs[s].ld >= F;
        const unsigned long long b =
            __ballot(valid && p != GNN_PLACE_HOST && s_of == (unsigned)s && live && slot < srcs[s].rows);
        if (lane == s) cnt += __popcll(b);
      }
      if (lane == nsrc && host) cnt += __popcll(hm);
    }
    while (hm) {
      const int b0 = __builtin_ctzll(hm);
      hm &= hm - 1;
      const int b1 = hm ? __builtin_ctzll(hm) : b0;  // an odd last row is simply copied twice
      hm &= hm - 1;  // (0 stays 0)
      float* d0 = dst + (i0 + b0) * ld_dst;
      float* d1 = dst + (i0 + b1) * ld_dst;
      if (!host) {  // host-placed nodes and no host table
        placed_zero_row(d0, F, lane, flag);
        placed_zero_row(d1, F, lane, flag);
        continue;
      }
      const E* s0 = host + (int64_t)__builtin_amdgcn_readlane(node, b0) * ld_host;
      const E* s1 = host + (int64_t)__builtin_amdgcn_readlane(node, b1) * ld_host;
      if (CAP >= 8 && vwh == 8) placed_pair<KIND, (CAP >= 8 ? 8 : 1)>(s0, s1, d0, d1, F, lane);
      else if (CAP >= 4 && vwh == 4) placed_pair<KIND, (CAP >= 4 ? 4 : 1)>(s0, s1, d0, d1, F, lane);
      else if (CAP >= 2 && vwh == 2) placed_pair<KIND, (CAP >= 2 ? 2 : 1)>(s0, s1, d0, d1, F, lane);
      else placed_pair<KIND, 1>(s0, s1, d0, d1, F, lane);
    }
  }
  if (counts && lane <= nsrc && cnt)
    __hip_atomic_fetch_add(counts + lane, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// What dst allows a load of fp32 / 16-bit source rows to be (pick_vw / pick_vw16's conditions on
// dst; F need not be a multiple: placed_row moves the columns after the last whole vector one per
// lane). The sources' own bases and strides are the kernel's to check, per source.
int placed_cap(int kind, int64_t ld_dst, const void* dst) {
  const uintptr_t pd = (uintptr_t)dst;
  const bool d4 = ld_dst % 4 == 0 && pd % 16 == 0, d2 = ld_dst % 2 == 0 && pd % 8 == 0;
  if (kind == GNN_FEAT_F32) return d4 ? 4 : (d2 ? 2 : 1);
  return d4 ? 8 : (d2 ? 2 : 1);
}

}  // namespace

extern "C" {

int gnn_gather_rows_f32(const float* src, int64_t ld_src, const int64_t* src_idx, float* dst, int64_t ld_dst,
                        const int64_t* dst_idx, int64_t n, int64_t F, void* stream) {
  GNN_REQUIRE(n >= 0 && F >= 0, "gnn_gather_rows_f32: negative size");
  GNN_REQUIRE(F <= ld_src && F <= ld_dst, "gnn_gather_rows_f32: F exceeds a row stride");
  GNN_REQUIRE(F < INT_MAX, "gnn_gather_rows_f32: F too large");
  if (n == 0 || F == 0) return 0;
  GNN_REQUIRE(src && dst, "gnn_gather_rows_f32: NULL src/dst");
  hipStream_t st = (hipStream_t)stream;
  const int vw = pick_vw(F, ld_src, ld_dst, src, dst);
  const dim3 grid((unsigned)ceil_div(n, 4));
  auto launch = [&](auto kern) {
    kern<<<grid, dim3(256), 0, st>>>(src, ld_src, src_idx, dst, ld_dst, dst_idx, n, (int)F);
  };
  if (vw == 4) launch(gather_rows_kernel<4>);
  else if (vw == 2) launch(gather_rows_kernel<2>);
  else launch(gather_rows_kernel<1>);
  GNN_LAUNCHED("gather_rows_kernel");
  return 0;
}

int gnn_gather_rows2_f32(const float* src0, int64_t ld0, const int64_t* idx0, const int64_t* pos0, int64_t n0,
                         const float* src1, int64_t ld1, const int64_t* idx1, const int64_t* pos1, int64_t n1,
                         float* dst, int64_t ld_dst, int64_t F, void* stream) {
  GNN_REQUIRE(n0 >= 0 && n1 >= 0 && F >= 0, "gnn_gather_rows2_f32: negative size");
  GNN_REQUIRE(F < INT_MAX && n0 + n1 < (int64_t)INT_MAX * 4, "gnn_gather_rows2_f32: too large");
  if (n0 + n1 == 0 || F == 0) return 0;
  GNN_REQUIRE(dst && (n0 == 0 || src0) && (n1 == 0 || src1), "gnn_gather_rows2_f32: NULL src/dst");
  GNN_REQUIRE(F <= ld_dst && (n0 == 0 || F <= ld0) && (n1 == 0 || F <= ld1),
              "gnn_gather_rows2_f32: F exceeds a row stride");
  hipStream_t st = (hipStream_t)stream;
  // 16-byte loads when every row of both sources and of dst allows them
  int vw = pick_vw(F, n0 ? ld0 : ld1, ld_dst, n0 ? src0 : src1, dst);
  if (n0 && n1) vw = std::min(vw, pick_vw(F, ld1, ld_dst, src1, dst));
  const dim3 grid((unsigned)ceil_div(n0 + n1, (int64_t)4));
  const int per = (int)ceil_div(F, (int64_t)64 * vw);  // loads per lane
#define GNN_G2(VW, NL) \
  gather_rows2_kernel<VW, NL><<<grid, dim3(256), 0, st>>>(src0, ld0, idx0, pos0, n0, src1, ld1, idx1, pos1, n1, dst, ld_dst, (int)F)
  if (vw == 4 && per <= 3) GNN_G2(4, 3);
  else if (vw == 4 && per <= 8) GNN_G2(4, 8);
  else if (vw == 2 && per <= 8) GNN_G2(2, 8);
  else if (vw == 1 && per <= 16) GNN_G2(1, 16);
  else {  // wide rows: the one-source kernel per source
    const int rc = gnn_gather_rows_f32(src0, ld0, idx0, dst, ld_dst, pos0, n0, F, stream);
    if (rc) return rc;
    return gnn_gather_rows_f32(src1, ld1, idx1, dst, ld_dst, pos1, n1, F, stream);
  }
#undef GNN_G2
  GNN_LAUNCHED("gather_rows2_kernel");
  return 0;
}

#define GNN_H16_DISPATCH(LAUNCH)                             \
  do {                                                       \
    if (kind == GNN_FEAT_F16) {                              \
      if (vw == 8) LAUNCH(GNN_FEAT_F16, 8);                  \
      else if (vw == 4) LAUNCH(GNN_FEAT_F16, 4);             \
      else if (vw == 2) LAUNCH(GNN_FEAT_F16, 2);             \
      else LAUNCH(GNN_FEAT_F16, 1);                          \
    } else {                                                 \
      if (vw == 8) LAUNCH(GNN_FEAT_BF16, 8);                 \
      else if (vw == 4) LAUNCH(GNN_FEAT_BF16, 4);            \
      else if (vw == 2) LAUNCH(GNN_FEAT_BF16, 2);            \
      else LAUNCH(GNN_FEAT_BF16, 1);                         \
    }                                                        \
  } while (0)

int gnn_gather_rows_h16_f32(const void* src, int64_t ld_src, int kind, const int64_t* src_idx, float* dst,
                            int64_t ld_dst, const int64_t* dst_idx, int64_t n, int64_t F, void* stream) {
  GNN_REQUIRE(kind == GNN_FEAT_F16 || kind == GNN_FEAT_BF16, "gnn_gather_rows_h16_f32: kind %d is not a 16-bit kind",
              kind);
  GNN_REQUIRE(n >= 0 && F >= 0, "gnn_gather_rows_h16_f32: negative size");
  GNN_REQUIRE(F <= ld_src && F <= ld_dst, "gnn_gather_rows_h16_f32: F exceeds a row stride");
  GNN_REQUIRE(F <= ((int64_t)1 << 30) && n < (int64_t)INT_MAX * 4, "gnn_gather_rows_h16_f32: too large");
  if (n == 0 || F == 0) return 0;
  GNN_REQUIRE(src && dst, "gnn_gather_rows_h16_f32: NULL src/dst");
  GNN_REQUIRE((uintptr_t)src % 2 == 0 && (uintptr_t)dst % 4 == 0, "gnn_gather_rows_h16_f32: misaligned src/dst");
  hipStream_t st = (hipStream_t)stream;
  const unsigned short* s = (const unsigned short*)src;
  const int vw = pick_vw16(F, ld_src, ld_dst, src, dst);
  const dim3 grid((unsigned)ceil_div(n, (int64_t)4));
#define GNN_H1(KIND, VW) \
  gather_rows_h16_kernel<KIND, VW, h16_nl(VW)><<<grid, dim3(256), 0, st>>>(s, ld_src, src_idx, dst, ld_dst, dst_idx, n, (int)F)
  GNN_H16_DISPATCH(GNN_H1);
#undef GNN_H1
  GNN_LAUNCHED("gather_rows_h16_kernel");
  return 0;
}

int gnn_gather_rows2_h16_f32(const void* src0, int64_t ld0, const int64_t* idx0, const int64_t* pos0, int64_t n0,
                             const void* src1, int64_t ld1, const int64_t* idx1, const int64_t* pos1, int64_t n1,
                             int kind, float* dst, int64_t ld_dst, int64_t F, void* stream) {
  GNN_REQUIRE(kind == GNN_FEAT_F16 || kind == GNN_FEAT_BF16, "gnn_gather_rows2_h16_f32: kind %d is not a 16-bit kind",
              kind);
  GNN_REQUIRE(n0 >= 0 && n1 >= 0 && F >= 0, "gnn_gather_rows2_h16_f32: negative size");
  GNN_REQUIRE(F <= ((int64_t)1 << 30) && n0 < (int64_t)INT_MAX * 2 && n1 < (int64_t)INT_MAX * 2,
              "gnn_gather_rows2_h16_f32: too large");
  if (n0 + n1 == 0 || F == 0) return 0;
  GNN_REQUIRE(dst && (n0 == 0 || src0) && (n1 == 0 || src1), "gnn_gather_rows2_h16_f32: NULL src/dst");
  GNN_REQUIRE(F <= ld_dst && (n0 == 0 || F <= ld0) && (n1 == 0 || F <= ld1),
              "gnn_gather_rows2_h16_f32: F exceeds a row stride");
  GNN_REQUIRE((n0 == 0 || (uintptr_t)src0 % 2 == 0) && (n1 == 0 || (uintptr_t)src1 % 2 == 0) && (uintptr_t)dst % 4 == 0,
              "gnn_gather_rows2_h16_f32: misaligned src/dst");
  hipStream_t st = (hipStream_t)stream;
  const unsigned short* s0 = (const unsigned short*)src0;
  const unsigned short* s1 = (const unsigned short*)src1;
  // the widest load that every row of both sources and of dst allows
  int vw = pick_vw16(F, n0 ? ld0 : ld1, ld_dst, n0 ? src0 : src1, dst);
  if (n0 && n1) vw = std::min(vw, pick_vw16(F, ld1, ld_dst, src1, dst));
  if (F > (int64_t)64 * vw * h16_nl(vw)) {  // wide rows: the one-source kernel per source
    const int rc = n0 ? gnn_gather_rows_h16_f32(src0, ld0, kind, idx0, dst, ld_dst, pos0, n0, F, stream) : 0;
    if (rc || n1 == 0) return rc;
    return gnn_gather_rows_h16_f32(src1, ld1, kind, idx1, dst, ld_dst, pos1, n1, F, stream);
  }
  const dim3 grid((unsigned)ceil_div(n0 + n1, (int64_t)4));
#define GNN_H2(KIND, VW)                                                                                            \
  gather_rows2_h16_kernel<KIND, VW, h16_nl(VW)><<<grid, dim3(256), 0, st>>>(s0, ld0, idx0, pos0, n0, s1, ld1, idx1, \
                                                                            pos1, n1, dst, ld_dst, (int)F)
  GNN_H16_DISPATCH(GNN_H2);
#undef GNN_H2
  GNN_LAUNCHED("gather_rows2_h16_kernel");
  return 0;
}

int gnn_gather_rows_host_f32(const float* host_src, int64_t ld_src, const int64_t* src_idx, float* dst,
                             int64_t ld_dst, const int64_t* dst_idx, int64_t n, int64_t F, void* stream) {
  GNN_REQUIRE(n >= 0 && F >= 0, "gnn_gather_rows_host_f32: negative size");
  GNN_REQUIRE(F <= ld_src && F <= ld_dst, "gnn_gather_rows_host_f32: F exceeds a row stride");
  GNN_REQUIRE(F < INT_MAX, "gnn_gather_rows_host_f32: F too large");
  if (n == 0 || F == 0) return 0;
  GNN_REQUIRE(host_src && dst, "gnn_gather_rows_host_f32: NULL src/dst");
  void* dsrc = nullptr;
  GNN_HIP(hipHostGetDevicePointer(&dsrc, (void*)host_src, 0),
          "hipHostGetDevicePointer (host_src must be pinned, device-mapped host memory)");
  const float* src = (const float*)dsrc;
  hipStream_t st = (hipStream_t)stream;
  const int vw = pick_vw(F, ld_src, ld_dst, src, dst);
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n, 8), HOST_GATHER_GRID));
  auto launch = [&](auto kern) {
    kern<<<grid, dim3(256), 0, st>>>(src, ld_src, src_idx, dst, ld_dst, dst_idx, n, (int)F);
  };
  if (vw == 4) launch(gather_rows_host_kernel<4>);
  else if (vw == 2) launch(gather_rows_host_kernel<2>);
  else launch(gather_rows_host_kernel<1>);
  GNN_LAUNCHED("gather_rows_host_kernel");
  return 0;
}

int gnn_gather_placed_f32(const int32_t* place, int64_t num_nodes, const gnn_place_src* srcs, int nsrc,
                          const void* host_table, int64_t ld_host, int kind, const int32_t* nodes, int64_t n,
                          float* dst, int64_t ld_dst, int64_t F, int64_t* counts, int32_t* flag, void* stream) {
  GNN_REQUIRE(kind == GNN_FEAT_F32 || kind == GNN_FEAT_F16 || kind == GNN_FEAT_BF16,
              "gnn_gather_placed_f32: unknown kind %d", kind);
  GNN_REQUIRE(nsrc >= 1 && nsrc <= GNN_PLACE_MAX_SRC, "gnn_gather_placed_f32: nsrc %d outside [1, %d]", nsrc,
              GNN_PLACE_MAX_SRC);
  GNN_REQUIRE(num_nodes >= 0 && n >= 0 && F >= 0 && ld_dst >= 0 && ld_host >= 0,
              "gnn_gather_placed_f32: negative size");
  GNN_REQUIRE(num_nodes < INT_MAX && n < INT_MAX && F < INT_MAX, "gnn_gather_placed_f32: a size of 2^31 or more");
  GNN_REQUIRE(F <= ld_dst && (host_table == nullptr || F <= ld_host),
              "gnn_gather_placed_f32: F exceeds a row stride");
  if (n == 0 || F == 0) return 0;
  GNN_REQUIRE(place && srcs && nodes && dst && flag, "gnn_gather_placed_f32: NULL place/srcs/nodes/dst/flag");
  const size_t esz = kind == GNN_FEAT_F32 ? 4 : 2;
  GNN_REQUIRE((uintptr_t)host_table % esz == 0 && (uintptr_t)dst % 4 == 0,
              "gnn_gather_placed_f32: misaligned host_table/dst");
  const void* host = nullptr;
  if (host_table) {
    void* d = nullptr;
    GNN_HIP(hipHostGetDevicePointer(&d, (void*)host_table, 0),
            "hipHostGetDevicePointer (host_table must be pinned, device-mapped host memory)");
    host = d;
  }
  hipStream_t st = (hipStream_t)stream;
  const int walkers = (int)std::min<int64_t>(ceil_div(n, (int64_t)256), HOST_GATHER_GRID);
  const dim3 grid((unsigned)(walkers + ceil_div(n, (int64_t)4)));
  const int cap = placed_cap(kind, ld_dst, dst);
#define GNN_GP(KIND, CAP)                                                                                        \
  gather_placed_kernel<KIND, CAP><<<grid, dim3(256), 0, st>>>(place, (int)num_nodes, srcs, nsrc, host, ld_host, \
                                                              nodes, n, dst, ld_dst, (int)F, counts, flag, walkers)
  if (kind == GNN_FEAT_F32) {
    if (cap == 4) GNN_GP(GNN_FEAT_F32, 4);
    else if (cap == 2) GNN_GP(GNN_FEAT_F32, 2);
    else GNN_GP(GNN_FEAT_F32, 1);
  } else {
    const int vw = cap;
    GNN_H16_DISPATCH(GNN_GP);
  }
#undef GNN_GP
  GNN_LAUNCHED("gather_placed_kernel");
  return 0;
}

}  // extern "C"
