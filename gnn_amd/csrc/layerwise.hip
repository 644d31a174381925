// layerwise.hip — the LADIES layer draw on the device, a hashed race over the resident graph
// (include/gnn_extract.h: gnn_lw_*, where the draw is stated in full).
//
// The reference draws a layer's columns with np.random.choice(p = U's column counts / their sum,
// replace = False): successive sampling without replacement, proportional to integer weights. The
// same law comes from a race: every entry of U gets an independent uniform 64-bit value, every
// column the maximum over its entries, and the s_num columns with the largest maxima are the draw.
// The values are a bijective hash of (column node id, row position) under a key of (seed, layer),
// so they are distinct, no tie rule exists, and the draw is a pure integer function of the seed.
//
// Launches, all on the caller's stream, stream order the only synchronisation between workgroups:
//   gnn_lw_race    memsets (count, key, total), then lw_race: a wave per row, grid-stride, the row's
//                  entries over the lanes (cl_mark's walk; waves never wait for one another, so a
//                  row of 10^5 entries holds up nobody). Per entry one table lookup (the column's
//                  position in the table), one 32-bit add and one 64-bit max, relaxed agent-scope
//                  atomics whose results are unused. A row's columns are distinct, so the lanes of
//                  one atomic instruction never collide. Add and max commute: the result does not
//                  depend on the schedule.
//   gnn_lw_select  an exact radix select over the full 64 bits, eight passes of eight bits from the
//                  top: lw_select_pass p first advances the state (prefix, keys still wanted) from
//                  pass p-1's 256-bin histogram — every workgroup on its own, workgroup 0 stores it
//                  — then adds its LDS histogram of digit p over the keys that match the prefix to
//                  the global one. lw_select_write advances once more (the prefix is then tau, the
//                  s_num-th largest key) and writes the ids. Pass 0 counts the live keys (count > 0
//                  among the table's members), so nlive and s_num are known from pass 1 on. The
//                  table's size is read from device memory; the grid is sized by the host's bound
//                  cap and nothing at or past the table's size is read.
//   gnn_lw_finish  lw_chunk_scan (blockIdx.y = which scan; closure.hip's cl_chunk_scan shape; also
//                  normfact and the exact 64-bit totals), scan_exclusive over the chunk sums of each
//                  scan, lw_chunk_add (offsets, the closing entries, the totals and their clamp).
// The subgraph sampler's square operand S = lap[after, :][:, after] (gnn_sg_*) needs two things more:
//   gnn_sg_count   sg_count: a wave per member of after, grid-stride, lap^T's row of that node over
//                  the lanes; each lane tests its entry against after's table and the wave sums the
//                  ballots' popcounts: S's column counts without an atomic, whatever the schedule.
//   gnn_sg_finish  the same three scan launches over two other sources (the column counts, and
//                  deg(after) with its offsets this time).
// The locality-skewed draw (gnn_lw_race_skew / gnn_lw_finish_skew: a favoured bit table and an integer
// scale) gives an entry of a favoured column `scale` replicas; the race takes their maximum in
// registers after one 4-byte read of the column's favoured word, and finish weighs normfact by
// count * s(c). The plain entry points are the skewed ones with (NULL, 1): the unskewed instantiation.
// Memory safety does not depend on the contents of the device arrays: a row id outside the graph,
// a row pointer outside [0, num_entries] or running backwards, a column outside the live table or
// at a position >= cap contribute nothing; device-side sizes (the table's, K) are clamped to the host's
// capacities. Each such case ORs 1 into err_flag.
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
using gnn::table_pos;

using Word = uint2;  // extract.hip's membership word
using u64 = unsigned long long;
using i64 = long long;

constexpr int LW_ITEMS = 8;
constexpr int LW_CHUNK = 1024 * LW_ITEMS;  // entries per scan workgroup
constexpr int LW_RACE_WAVES = 4;           // waves per racing workgroup
constexpr int LW_RACE_GRID = 4096;         // at most this many racing workgroups
constexpr int LW_BINS = 256;               // one radix digit: 8 bits
constexpr int LW_PASSES = 8;
constexpr int LW_SEL_ITEMS = 8;            // keys per thread a select workgroup is sized for
constexpr int LW_SEL_GRID = 1024;          // at most this many select workgroups
constexpr int LW_SCANS = 3;                // colptr_t, rowseg, colseg (a fourth sum has no offsets)
constexpr int SG_SCANS = 2;                // the square operand's colptr_t and rowseg

// What a slot (blockIdx.y) of the chunk scans sums: count[after[k]] through the live table (and
// normfact), deg(rows[i]), lap^T's row length of after[k], deg(after[k]), colcnt[k] as it stands.
enum ScanSrc : int { SRC_COUNT = 0, SRC_DEG_ROWS = 1, SRC_DEGT_AFTER = 2, SRC_DEG_AFTER = 3, SRC_COLCNT = 4 };

__host__ __device__ __forceinline__ u64 mix64(u64 z) {  // the splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// s(c) of the skewed draw: `scale` for a node of the favoured bit table (bit c & 31 of word c >> 5),
// else 1. c has passed table_pos, so 0 <= c < N and the word lies inside the table.
__device__ __forceinline__ int lw_replicas(const uint32_t* __restrict__ favoured, int scale, int c) {
  return ((favoured[c >> 5] >> ((unsigned)c & 31u)) & 1u) ? scale : 1;
}

// SKEW: an entry of a favoured column races with `scale` replicas, replica r under the value
// mix64((c << 32 | r << 26 | i) + K) (M < 2^26, the host has checked); their maximum is taken in
// registers, so an entry still costs one add and one max. The wave adds s(c) per entry to total.
template <bool SKEW>
__global__ __launch_bounds__(64 * LW_RACE_WAVES) void lw_race_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int N, int64_t E,
    const int32_t* __restrict__ rows, int M, const Word* __restrict__ live, u64 K, int32_t* __restrict__ count,
    u64* __restrict__ key, int cap, i64* __restrict__ total, int32_t* __restrict__ err,
    const uint32_t* __restrict__ favoured, int scale) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * LW_RACE_WAVES + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * LW_RACE_WAVES;
  i64 mine = 0;
  bool bad = false;
  for (int64_t i = wave; i < M; i += nwaves) {
    int64_t b;
    int d;
    bad |= !row_span(indptr, N, E, rows[i], b, d);
    for (int k = lane; k < d; k += 64) {
      const int c = indices[b + k];
      const int p = table_pos(live, N, c);
      if (p < 0 || p >= cap) {  // not a column of the live table the caller made of these rows
        bad = true;
        continue;
      }
      u64 h = mix64((((u64)(uint32_t)c << 32) | (u64)(uint32_t)i) + K);
      if constexpr (SKEW) {
        const int s = lw_replicas(favoured, scale, c);
        for (int r = 1; r < s; ++r) {
          const u64 hr = mix64((((u64)(uint32_t)c << 32) | ((u64)r << 26) | (u64)(uint32_t)i) + K);
          h = hr > h ? hr : h;
        }
        mine += s;
      } else {
        ++mine;
      }
      (void)__hip_atomic_fetch_add(&count[p], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_max(&key[p], h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
  if (lane == 0 && mine) (void)__hip_atomic_fetch_add(total, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (__ballot(bad) && lane == 0 && err) atomicOr(err, 1);
}

// The select's state before a pass: the digits fixed so far (in place, from the top), how many of
// the live keys that match them are still wanted — the answer is the krem-th largest of those —
// and s_num, carried along.
struct SelState {
  u64 prefix;
  i64 krem;
  i64 snum;
  i64 pad;
};

__device__ __forceinline__ int64_t clamp_size(const int64_t* p, int64_t cap) {
  const int64_t n = *p;
  return n < 0 ? 0 : (n > cap ? cap : n);
}

// The state before pass `pass` (1 .. LW_PASSES), computed by all 256 threads of a workgroup from
// the state before pass - 1 and that pass's histogram: the bin b with (keys in higher bins) < krem
// <= (those + hist[b]) is the next digit. Pass 0 counts every live key, so the sum of its
// histogram is nlive and the state before it (no digit, s_num = min(nlive, samp_num) wanted) is
// made here as well. Before pass 0 nothing is known and nothing is needed.
__device__ __forceinline__ SelState sel_advance(int pass, const unsigned* __restrict__ hist,
                                                const SelState* __restrict__ state, int64_t samp) {
  __shared__ unsigned suf[LW_BINS];
  __shared__ SelState cur;
  const int tid = threadIdx.x;
  if (pass == 0) return SelState{0ull, 0, 0, 0};  // block-uniform
  SelState prev = state[pass - 1];
  const unsigned h = hist[(pass - 1) * LW_BINS + tid];
  suf[tid] = h;
  __syncthreads();
  for (int d = 1; d < LW_BINS; d <<= 1) {  // inclusive suffix sums
    const unsigned v = tid + d < LW_BINS ? suf[tid + d] : 0u;
    __syncthreads();
    suf[tid] += v;
    __syncthreads();
  }
  if (pass == 1) {
    const i64 nlive = (i64)suf[0];
    prev = SelState{0ull, nlive < samp ? nlive : samp, nlive < samp ? nlive : samp, 0};
  }
  const i64 above = (i64)(suf[tid] - h);
  if (tid == 0) cur = prev;  // nothing wanted (krem = 0): nothing moves
  __syncthreads();
  if (prev.krem > 0 && above < prev.krem && prev.krem <= above + (i64)h)
    cur = SelState{prev.prefix | ((u64)tid << (64 - 8 * pass)), prev.krem - above, prev.snum, 0};
  __syncthreads();
  return cur;
}

// count[j] > 0 marks the live positions of the table (its other members are rows that are nobody's
// column: key 0, never drawn)
__global__ __launch_bounds__(LW_BINS) void lw_select_pass_kernel(const u64* __restrict__ key,
                                                                 const int32_t* __restrict__ count,
                                                                 const int64_t* __restrict__ ntab, int64_t cap,
                                                                 int64_t samp, int pass, unsigned* __restrict__ hist,
                                                                 SelState* __restrict__ state) {
  __shared__ unsigned lh[LW_BINS];
  const int tid = threadIdx.x;
  const int64_t n = clamp_size(ntab, cap);
  const SelState s = sel_advance(pass, hist, state, samp);
  if (blockIdx.x == 0 && tid == 0) state[pass] = s;
  lh[tid] = 0u;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  for (int64_t j = (int64_t)blockIdx.x * LW_BINS + tid; j < n; j += (int64_t)gridDim.x * LW_BINS) {
    if (count[j] <= 0) continue;
    const u64 k = key[j];
    if (pass == 0 || ((k ^ s.prefix) >> (shift + 8)) == 0) atomicAdd(&lh[(unsigned)(k >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (lh[tid])
    (void)__hip_atomic_fetch_add(&hist[pass * LW_BINS + tid], lh[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(LW_BINS) void lw_select_write_kernel(const u64* __restrict__ key,
                                                                  const int32_t* __restrict__ count,
                                                                  const int64_t* __restrict__ ntab, int64_t cap,
                                                                  int64_t samp, const unsigned* __restrict__ hist,
                                                                  const SelState* __restrict__ state,
                                                                  const int32_t* __restrict__ tab_ids,
                                                                  int32_t* __restrict__ ids, int64_t* __restrict__ s_num,
                                                                  u64* __restrict__ tau) {
  const int tid = threadIdx.x;
  const int64_t n = clamp_size(ntab, cap);
  const SelState s = sel_advance(LW_PASSES, hist, state, samp);
  const int64_t sn = s.snum;
  const u64 t = sn > 0 ? s.prefix : 0ull;
  if (blockIdx.x == 0 && tid == 0) {
    *s_num = sn;
    *tau = t;
  }
  for (int64_t j = (int64_t)blockIdx.x * LW_BINS + tid; j < cap; j += (int64_t)gridDim.x * LW_BINS)
    ids[j] = (sn > 0 && j < n && count[j] > 0 && key[j] >= t) ? tab_ids[j] : -1;
}

// normfact of a column of weight w (its entry count, times s(c) in the skewed draw) among a total
// weight of total, s_num columns drawn: the reference's 1 / float32(clip(s_num * p, 1e-10, 1)) with
// p = w / total in fp64 (0 when nothing was counted)
__device__ __forceinline__ float lw_normfact(i64 w, i64 total, i64 s_num) {
  double q = total > 0 ? (double)s_num * ((double)w / (double)total) : 0.0;
  q = q < 1e-10 ? 1e-10 : (q > 1.0 ? 1.0 : q);
  return 1.0f / (float)q;
}

struct FinishArgs {
  const int64_t* indptr;
  const int64_t* indptr_t;
  int64_t E, E_t;
  int N;
  const int32_t* rows;
  int M;
  const int32_t* after;
  const int64_t* K;
  int kcap;
  const Word* live;
  const int32_t* count;
  int cap;
  const i64* total;
  const i64* s_num;
  float* normfact;
  const int32_t* colcnt;   // SRC_COLCNT's values (gnn_sg_finish)
  int src[LW_SCANS + 1];   // per slot, a ScanSrc
  int nscan;               // slots below it have offsets (out[slot]); the others only a sum
  int32_t* out[LW_SCANS];  // gnn_lw_finish: colptr_t, rowseg, colseg
  int32_t* csum;           // [nscan][cstride]
  int32_t* coff;           // [nscan][cstride]
  int cstride, nch;
  i64* tot;                // [4]: the slots' sums, exact
  int64_t* totals;         // the caller's totals: totals[j] = tot[totmap[j]], j < ntot, clamped
  int ntot, totmap[3];
  int32_t* err;
  const uint32_t* favoured;  // the skewed draw's bit table, or NULL: every weight is the count
  int scale;
};

// blockIdx.y = which slot, a.src[which] what it sums (gnn_lw_finish: count[after[k]] and normfact,
// deg(rows[i]), lap^T's row length of after[k], and deg(after[k]) as a sum only). Offsets within the
// chunk go to out[which], the chunk's sum to csum (32-bit, wrapping; the exact sum goes to
// tot[which], which decides in lw_chunk_add).
__global__ __launch_bounds__(1024) void lw_chunk_scan_kernel(FinishArgs a) {
  __shared__ unsigned wsum[16];
  const int which = blockIdx.y, src = a.src[which];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * LW_CHUNK + (int64_t)tid * LW_ITEMS;
  const int n = src == SRC_DEG_ROWS ? a.M : (int)clamp_size(a.K, a.kcap);
  unsigned v[LW_ITEMS];
  unsigned tsum = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < LW_ITEMS; ++k) {
    v[k] = 0;
    if (base + k < n) {
      int64_t b;
      int d = 0;
      if (src == SRC_COUNT) {
        const int p = table_pos(a.live, a.N, a.after[base + k]);
        d = (p >= 0 && p < a.cap) ? a.count[p] : 0;
        if (d < 0) d = 0;
        i64 w = d;  // p >= 0: after[base + k] lies in [0, N), inside the favoured table
        if (a.favoured && d > 0) w *= lw_replicas(a.favoured, a.scale, a.after[base + k]);
        a.normfact[base + k] = lw_normfact(w, *a.total, *a.s_num);
      } else if (src == SRC_DEG_ROWS) {
        bad |= !row_span(a.indptr, a.N, a.E, a.rows[base + k], b, d);
      } else if (src == SRC_DEGT_AFTER) {
        bad |= !row_span(a.indptr_t, a.N, a.E_t, a.after[base + k], b, d);
      } else if (src == SRC_DEG_AFTER) {
        bad |= !row_span(a.indptr, a.N, a.E, a.after[base + k], b, d);
      } else {
        d = a.colcnt[base + k];
        if (d < 0) d = 0;
      }
      v[k] = (unsigned)d;
    }
    tsum += v[k];
  }
  if (bad && a.err) atomicOr(a.err, 1);
  i64 exact = 0;
#pragma unroll
  for (int k = 0; k < LW_ITEMS; ++k) exact += (i64)v[k];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) exact += __shfl_down(exact, d);
  if (lane == 0 && exact) (void)__hip_atomic_fetch_add(&a.tot[which], exact, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (which >= a.nscan) return;  // block-uniform
  unsigned x = tsum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  if (wave == 0) {
    unsigned w = lane < 16 ? wsum[lane] : 0u;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const unsigned y = __shfl_up(w, d);
      if (lane >= d) w += y;
    }
    if (lane < 16) wsum[lane] = w;
  }
  __syncthreads();
  unsigned excl = (wave ? wsum[wave - 1] : 0u) + x - tsum;
  int32_t* out = a.out[which];
#pragma unroll
  for (int k = 0; k < LW_ITEMS; ++k) {
    if (base + k < n) out[base + k] = (int32_t)excl;
    excl += v[k];
  }
  if (tid == 0) a.csum[which * a.cstride + blockIdx.x] = (int32_t)wsum[15];
}

// offsets += the chunk's start; thread n writes the closing entry. A sum of 2^31 or more raises
// the flag and leaves zero offsets; thread n of slot 0 also writes the caller's totals, clamped.
__global__ __launch_bounds__(256) void lw_chunk_add_kernel(FinishArgs a) {
  const int which = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = a.src[which] == SRC_DEG_ROWS ? a.M : (int)clamp_size(a.K, a.kcap);
  if (i > n) return;
  const bool over = a.tot[which] > (i64)INT_MAX;
  int32_t* out = a.out[which];
  const int32_t* coff = a.coff + which * a.cstride;
  if (i < n) {
    out[i] = over ? 0 : out[i] + coff[i / LW_CHUNK];
    return;
  }
  out[n] = over ? 0 : coff[a.nch];
  bool flag = over;
  if (which == 0) {
    for (int j = 0; j < a.ntot; ++j) {
      const i64 t = a.tot[a.totmap[j]];
      a.totals[j] = t > INT_MAX ? INT_MAX : t;
      flag |= t > (i64)INT_MAX;  // a sum-only slot has no thread of its own here
    }
    flag |= *a.K != (int64_t)n;  // the set does not fit the caller's capacity
  }
  if (flag && a.err) atomicOr(a.err, 1);
}

// S's column counts: colcnt[k] = the entries of lap^T's row after[k] that are members of after's
// table. A wave per k, grid-stride; the trip count is wave-uniform, so every ballot sees all lanes.
__global__ __launch_bounds__(64 * LW_RACE_WAVES) void sg_count_kernel(
    const int64_t* __restrict__ indptr_t, const int32_t* __restrict__ indices_t, int N, int64_t E_t,
    const int32_t* __restrict__ after, const int64_t* __restrict__ K, int kcap, const Word* __restrict__ table,
    int32_t* __restrict__ colcnt, int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * LW_RACE_WAVES + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * LW_RACE_WAVES;
  const int64_t n = clamp_size(K, kcap);
  bool bad = false;
  for (int64_t k = wave; k < n; k += nwaves) {
    int64_t b;
    int d;
    bad |= !row_span(indptr_t, N, E_t, after[k], b, d);
    int cnt = 0;
    for (int e = 0; e < d; e += 64) {  // d < 2^31 - 1: the sum fits
      const bool member = e + lane < d && table_pos(table, N, indices_t[b + e + lane]) >= 0;
      cnt += __popcll(__ballot(member));
    }
    if (lane == 0) colcnt[k] = cnt;
  }
  if (__ballot(bad) && lane == 0 && err) atomicOr(err, 1);
}

inline size_t csum_bytes(int64_t n) {
  return align_up(((size_t)ceil_div(n, (int64_t)LW_CHUNK) + 1) * sizeof(int32_t), 256);
}

// What the two skewed entry points refuse of (favoured, scale): replica r sits in bits 26 .. 31 of
// the hashed word and the row position below it, hence scale <= 64 and M < 2^26 where replicas race.
inline int skew_ok(const char* fn, const uint32_t* favoured, int32_t scale, int64_t M) {
  GNN_REQUIRE(scale >= 1 && scale <= 64, "%s: scale %d outside [1, 64]", fn, (int)scale);
  GNN_REQUIRE((uintptr_t)favoured % 4 == 0, "%s: favoured table not 4-byte aligned", fn);
  GNN_REQUIRE(!(favoured && scale > 1) || M < ((int64_t)1 << 26),
              "%s: a skewed race needs M < 2^26 rows (the row position shares a word with the replica)", fn);
  return 0;
}

constexpr size_t SEL_HIST_BYTES = (size_t)LW_PASSES * LW_BINS * sizeof(unsigned);
constexpr size_t SEL_STATE_BYTES = (size_t)(LW_PASSES + 1) * sizeof(SelState);

}  // namespace

extern "C" {

int gnn_lw_race(const int64_t* indptr, const int32_t* indices, int64_t num_nodes, int64_t num_entries,
                const int32_t* rows, int64_t M, const void* live_table, uint64_t seed, int32_t layer, int32_t* count,
                uint64_t* key, int64_t cap, int64_t* total, int32_t* err_flag, void* stream) {
  return gnn_lw_race_skew(indptr, indices, num_nodes, num_entries, rows, M, live_table, seed, layer, count, key, cap,
                          total, err_flag, stream, nullptr, 1);
}

int gnn_lw_race_skew(const int64_t* indptr, const int32_t* indices, int64_t num_nodes, int64_t num_entries,
                     const int32_t* rows, int64_t M, const void* live_table, uint64_t seed, int32_t layer,
                     int32_t* count, uint64_t* key, int64_t cap, int64_t* total, int32_t* err_flag, void* stream,
                     const uint32_t* favoured, int32_t scale) {
  GNN_REQUIRE(num_nodes >= 0 && num_entries >= 0 && M >= 0 && cap >= 0,
              "gnn_lw_race: negative size (num_nodes, num_entries, M or cap)");
  GNN_REQUIRE(num_nodes < INT_MAX && M < INT_MAX && cap < INT_MAX, "gnn_lw_race: num_nodes, M and cap must be < 2^31");
  GNN_REQUIRE(layer >= 0, "gnn_lw_race: negative layer");
  GNN_REQUIRE(total != nullptr, "gnn_lw_race: NULL total");
  GNN_REQUIRE(live_table != nullptr, "gnn_lw_race: NULL live table");
  GNN_REQUIRE((uintptr_t)live_table % 8 == 0, "gnn_lw_race: live table not 8-byte aligned");
  GNN_REQUIRE(cap == 0 || (count && key), "gnn_lw_race: NULL count/key");
  GNN_REQUIRE((uintptr_t)key % 8 == 0 && (uintptr_t)total % 8 == 0, "gnn_lw_race: key/total not 8-byte aligned");
  GNN_REQUIRE(M == 0 || (indptr && rows), "gnn_lw_race: NULL indptr/rows");
  GNN_REQUIRE(M == 0 || num_entries == 0 || indices, "gnn_lw_race: NULL indices");
  int rc = skew_ok("gnn_lw_race_skew", favoured, scale, M);
  if (rc) return rc;
  const bool skew = favoured != nullptr && scale > 1;
  hipStream_t st = (hipStream_t)stream;
  GNN_HIP(hipMemsetAsync(total, 0, sizeof(int64_t), st), "hipMemsetAsync");
  if (cap > 0) {
    GNN_HIP(hipMemsetAsync(count, 0, (size_t)cap * sizeof(int32_t), st), "hipMemsetAsync");
    GNN_HIP(hipMemsetAsync(key, 0, (size_t)cap * sizeof(uint64_t), st), "hipMemsetAsync");
  }
  if (M == 0) return 0;
  const u64 K = mix64((u64)seed + ((u64)layer + 1ull) * 0x9E3779B97F4A7C15ull);
  const int64_t g = ceil_div(M, (int64_t)LW_RACE_WAVES);
  const dim3 grid((unsigned)(g < LW_RACE_GRID ? g : LW_RACE_GRID)), block(64 * LW_RACE_WAVES);
  if (skew)
    lw_race_kernel<true><<<grid, block, 0, st>>>(indptr, indices, (int)num_nodes, num_entries, rows, (int)M,
                                                 (const Word*)live_table, K, count, (u64*)key, (int)cap, (i64*)total,
                                                 err_flag, favoured, scale);
  else
    lw_race_kernel<false><<<grid, block, 0, st>>>(indptr, indices, (int)num_nodes, num_entries, rows, (int)M,
                                                  (const Word*)live_table, K, count, (u64*)key, (int)cap, (i64*)total,
                                                  err_flag, nullptr, 1);
  GNN_LAUNCHED("lw_race_kernel");
  return 0;
}

size_t gnn_lw_select_workspace_bytes(void) { return align_up(SEL_HIST_BYTES + SEL_STATE_BYTES, 256); }

int gnn_lw_select(const uint64_t* key, const int32_t* count, const int64_t* ntab, int64_t cap, int64_t samp_num,
                  const int32_t* tab_ids, int32_t* ids, int64_t* s_num, uint64_t* tau, void* workspace, size_t workspace_bytes, void* stream) {
  GNN_REQUIRE(cap >= 0, "gnn_lw_select: negative cap");
  GNN_REQUIRE(cap < INT_MAX, "gnn_lw_select: cap must be < 2^31");
  GNN_REQUIRE(samp_num >= 1, "gnn_lw_select: samp_num must be >= 1");
  GNN_REQUIRE(ntab && s_num && tau, "gnn_lw_select: NULL ntab/s_num/tau");
  GNN_REQUIRE(cap == 0 || (key && count && tab_ids && ids), "gnn_lw_select: NULL key/count/tab_ids/ids");
  GNN_REQUIRE((uintptr_t)key % 8 == 0 && (uintptr_t)ntab % 8 == 0 && (uintptr_t)s_num % 8 == 0 &&
                  (uintptr_t)tau % 8 == 0,
              "gnn_lw_select: key/ntab/s_num/tau not 8-byte aligned");
  const size_t need = gnn_lw_select_workspace_bytes();
  GNN_REQUIRE(workspace && workspace_bytes >= need, "gnn_lw_select: workspace too small (%zu < %zu)",
              workspace ? workspace_bytes : (size_t)0, need);
  GNN_REQUIRE((uintptr_t)workspace % 16 == 0, "gnn_lw_select: workspace not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  unsigned* hist = (unsigned*)workspace;
  SelState* state = (SelState*)((char*)workspace + SEL_HIST_BYTES);
  GNN_HIP(hipMemsetAsync(workspace, 0, SEL_HIST_BYTES + SEL_STATE_BYTES, st), "hipMemsetAsync");
  int64_t g = ceil_div(cap, (int64_t)LW_BINS * LW_SEL_ITEMS);
  g = g < 1 ? 1 : (g > LW_SEL_GRID ? LW_SEL_GRID : g);
  for (int pass = 0; pass < LW_PASSES; ++pass) {
    lw_select_pass_kernel<<<dim3((unsigned)g), dim3(LW_BINS), 0, st>>>((const u64*)key, count, ntab, cap, samp_num, pass,
                                                                      hist, state);
    GNN_LAUNCHED("lw_select_pass_kernel");
  }
  lw_select_write_kernel<<<dim3((unsigned)g), dim3(LW_BINS), 0, st>>>((const u64*)key, count, ntab, cap, samp_num, hist,
                                                                     state, tab_ids, ids, s_num, (u64*)tau);
  GNN_LAUNCHED("lw_select_write_kernel");
  return 0;
}

size_t gnn_lw_finish_workspace_bytes(int64_t M, int64_t kcap) {
  const int64_t n = M > kcap ? M : kcap;
  return 2 * LW_SCANS * csum_bytes(n > 0 ? n : 0) + 256;  // the chunk sums, their scans, the exact totals
}

int gnn_lw_finish(const int64_t* indptr, int64_t num_entries, const int64_t* indptr_t, int64_t num_entries_t,
                  int64_t num_nodes, const int32_t* rows, int64_t M, const int32_t* after, const int64_t* K,
                  int64_t kcap, const void* live_table, const int32_t* count, int64_t cap, const int64_t* total,
                  const int64_t* s_num, float* normfact, int32_t* colptr_t, int32_t* rowseg, int32_t* colseg,
                  int64_t* totals, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  return gnn_lw_finish_skew(indptr, num_entries, indptr_t, num_entries_t, num_nodes, rows, M, after, K, kcap, live_table,
                            count, cap, total, s_num, normfact, colptr_t, rowseg, colseg, totals, workspace,
                            workspace_bytes, err_flag, stream, nullptr, 1);
}

int gnn_lw_finish_skew(const int64_t* indptr, int64_t num_entries, const int64_t* indptr_t, int64_t num_entries_t,
                       int64_t num_nodes, const int32_t* rows, int64_t M, const int32_t* after, const int64_t* K,
                       int64_t kcap, const void* live_table, const int32_t* count, int64_t cap, const int64_t* total,
                       const int64_t* s_num, float* normfact, int32_t* colptr_t, int32_t* rowseg, int32_t* colseg,
                       int64_t* totals, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream,
                       const uint32_t* favoured, int32_t scale) {
  GNN_REQUIRE(num_nodes >= 0 && num_entries >= 0 && num_entries_t >= 0 && M >= 0 && kcap >= 0 && cap >= 0,
              "gnn_lw_finish: negative size (num_nodes, num_entries, num_entries_t, M, kcap or cap)");
  GNN_REQUIRE(num_nodes < INT_MAX && M < INT_MAX && kcap < INT_MAX && cap < INT_MAX,
              "gnn_lw_finish: num_nodes, M, kcap and cap must be < 2^31");
  GNN_REQUIRE(K && total && s_num && totals, "gnn_lw_finish: NULL K/total/s_num/totals");
  GNN_REQUIRE((uintptr_t)K % 8 == 0 && (uintptr_t)total % 8 == 0 && (uintptr_t)s_num % 8 == 0 &&
                  (uintptr_t)totals % 8 == 0,
              "gnn_lw_finish: K/total/s_num/totals not 8-byte aligned");
  GNN_REQUIRE(live_table != nullptr, "gnn_lw_finish: NULL live table");
  GNN_REQUIRE((uintptr_t)live_table % 8 == 0, "gnn_lw_finish: live table not 8-byte aligned");
  GNN_REQUIRE(colptr_t && rowseg && colseg, "gnn_lw_finish: NULL colptr_t/rowseg/colseg");
  GNN_REQUIRE(cap == 0 || count, "gnn_lw_finish: NULL count");
  GNN_REQUIRE(kcap == 0 || (after && normfact), "gnn_lw_finish: NULL after/normfact");
  GNN_REQUIRE(M == 0 || rows, "gnn_lw_finish: NULL rows");
  GNN_REQUIRE((M == 0 && kcap == 0) || (indptr && indptr_t), "gnn_lw_finish: NULL indptr/indptr_t");
  int src = skew_ok("gnn_lw_finish_skew", favoured, scale, M);
  if (src) return src;
  const size_t need = gnn_lw_finish_workspace_bytes(M, kcap);
  GNN_REQUIRE(workspace && workspace_bytes >= need, "gnn_lw_finish: workspace too small (%zu < %zu)",
              workspace ? workspace_bytes : (size_t)0, need);
  GNN_REQUIRE((uintptr_t)workspace % 16 == 0, "gnn_lw_finish: workspace not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = M > kcap ? M : kcap;
  const int nch = (int)ceil_div(n, (int64_t)LW_CHUNK);
  const size_t cb = csum_bytes(n);
  FinishArgs a;
  a.indptr = indptr;
  a.indptr_t = indptr_t;
  a.E = num_entries;
  a.E_t = num_entries_t;
  a.N = (int)num_nodes;
  a.rows = rows;
  a.M = (int)M;
  a.after = after;
  a.K = K;
  a.kcap = (int)kcap;
  a.live = (const Word*)live_table;
  a.count = count;
  a.cap = (int)cap;
  a.total = (const i64*)total;
  a.s_num = (const i64*)s_num;
  a.normfact = normfact;
  a.colcnt = nullptr;
  a.src[0] = SRC_COUNT, a.src[1] = SRC_DEG_ROWS, a.src[2] = SRC_DEGT_AFTER, a.src[3] = SRC_DEG_AFTER;
  a.nscan = LW_SCANS;
  a.ntot = 3, a.totmap[0] = 0, a.totmap[1] = 2, a.totmap[2] = 3;
  a.out[0] = colptr_t;
  a.out[1] = rowseg;
  a.out[2] = colseg;
  a.csum = (int32_t*)workspace;
  a.coff = (int32_t*)((char*)workspace + LW_SCANS * cb);
  a.cstride = (int)(cb / sizeof(int32_t));
  a.nch = nch;
  a.tot = (i64*)((char*)workspace + 2 * LW_SCANS * cb);
  a.totals = totals;
  a.err = err_flag;
  a.favoured = scale > 1 ? favoured : nullptr;
  a.scale = scale;
  GNN_HIP(hipMemsetAsync(a.tot, 0, 4 * sizeof(i64), st), "hipMemsetAsync");
  if (nch > 0) {
    lw_chunk_scan_kernel<<<dim3((unsigned)nch, LW_SCANS + 1), dim3(1024), 0, st>>>(a);
    GNN_LAUNCHED("lw_chunk_scan_kernel");
  }
  for (int w = 0; w < LW_SCANS; ++w) {
    int rc = gnn::launch_scan_exclusive(a.csum + w * a.cstride, nch, a.coff + w * a.cstride, st);
    if (rc) return rc;
  }
  lw_chunk_add_kernel<<<dim3((unsigned)ceil_div(n + 1, 256), LW_SCANS), dim3(256), 0, st>>>(a);
  GNN_LAUNCHED("lw_chunk_add_kernel");
  return 0;
}

int gnn_sg_count(const int64_t* indptr_t, const int32_t* indices_t, int64_t num_nodes, int64_t num_entries_t,
                 const int32_t* after, const int64_t* K, int64_t kcap, const void* table, int32_t* colcnt,
                 int32_t* err_flag, void* stream) {
  GNN_REQUIRE(num_nodes >= 0 && num_entries_t >= 0 && kcap >= 0,
              "gnn_sg_count: negative size (num_nodes, num_entries_t or kcap)");
  GNN_REQUIRE(num_nodes < INT_MAX && kcap < INT_MAX, "gnn_sg_count: num_nodes and kcap must be < 2^31");
  GNN_REQUIRE(K != nullptr, "gnn_sg_count: NULL K");
  GNN_REQUIRE((uintptr_t)K % 8 == 0, "gnn_sg_count: K not 8-byte aligned");
  GNN_REQUIRE(table != nullptr, "gnn_sg_count: NULL table");
  GNN_REQUIRE((uintptr_t)table % 8 == 0, "gnn_sg_count: table not 8-byte aligned");
  GNN_REQUIRE(kcap == 0 || (after && colcnt && indptr_t), "gnn_sg_count: NULL after/colcnt/indptr_t");
  GNN_REQUIRE(kcap == 0 || num_entries_t == 0 || indices_t, "gnn_sg_count: NULL indices_t");
  if (kcap == 0) return 0;
  const int64_t g = ceil_div(kcap, (int64_t)LW_RACE_WAVES);
  sg_count_kernel<<<dim3((unsigned)(g < LW_RACE_GRID ? g : LW_RACE_GRID)), dim3(64 * LW_RACE_WAVES), 0,
                    (hipStream_t)stream>>>(indptr_t, indices_t, (int)num_nodes, num_entries_t, after, K, (int)kcap,
                                           (const Word*)table, colcnt, err_flag);
  GNN_LAUNCHED("sg_count_kernel");
  return 0;
}

size_t gnn_sg_finish_workspace_bytes(int64_t kcap) {
  return 2 * SG_SCANS * csum_bytes(kcap > 0 ? kcap : 0) + 256;  // the chunk sums, their scans, the exact totals
}

int gnn_sg_finish(const int64_t* indptr, int64_t num_entries, int64_t num_nodes, const int32_t* after,
                  const int64_t* K, int64_t kcap, const int32_t* colcnt, int32_t* colptr_t, int32_t* rowseg,
                  int64_t* totals, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  GNN_REQUIRE(num_nodes >= 0 && num_entries >= 0 && kcap >= 0,
              "gnn_sg_finish: negative size (num_nodes, num_entries or kcap)");
  GNN_REQUIRE(num_nodes < INT_MAX && kcap < INT_MAX, "gnn_sg_finish: num_nodes and kcap must be < 2^31");
  GNN_REQUIRE(K && totals, "gnn_sg_finish: NULL K/totals");
  GNN_REQUIRE((uintptr_t)K % 8 == 0 && (uintptr_t)totals % 8 == 0, "gnn_sg_finish: K/totals not 8-byte aligned");
  GNN_REQUIRE(colptr_t && rowseg, "gnn_sg_finish: NULL colptr_t/rowseg");
  GNN_REQUIRE(kcap == 0 || (after && colcnt && indptr), "gnn_sg_finish: NULL after/colcnt/indptr");
  const size_t need = gnn_sg_finish_workspace_bytes(kcap);
  GNN_REQUIRE(workspace && workspace_bytes >= need, "gnn_sg_finish: workspace too small (%zu < %zu)",
              workspace ? workspace_bytes : (size_t)0, need);
  GNN_REQUIRE((uintptr_t)workspace % 16 == 0, "gnn_sg_finish: workspace not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nch = (int)ceil_div(kcap, (int64_t)LW_CHUNK);
  const size_t cb = csum_bytes(kcap);
  FinishArgs a = {};
  a.indptr = indptr;
  a.E = num_entries;
  a.N = (int)num_nodes;
  a.after = after;
  a.K = K;
  a.kcap = (int)kcap;
  a.colcnt = colcnt;
  a.src[0] = SRC_COLCNT, a.src[1] = SRC_DEG_AFTER;
  a.nscan = SG_SCANS;
  a.ntot = 2, a.totmap[0] = 0, a.totmap[1] = 1;
  a.out[0] = colptr_t;
  a.out[1] = rowseg;
  a.csum = (int32_t*)workspace;
  a.coff = (int32_t*)((char*)workspace + SG_SCANS * cb);
  a.cstride = (int)(cb / sizeof(int32_t));
  a.nch = nch;
  a.tot = (i64*)((char*)workspace + 2 * SG_SCANS * cb);
  a.totals = totals;
  a.err = err_flag;
  GNN_HIP(hipMemsetAsync(a.tot, 0, 4 * sizeof(i64), st), "hipMemsetAsync");
  if (nch > 0) {
    lw_chunk_scan_kernel<<<dim3((unsigned)nch, SG_SCANS), dim3(1024), 0, st>>>(a);
    GNN_LAUNCHED("lw_chunk_scan_kernel");
  }
  for (int w = 0; w < SG_SCANS; ++w) {
    int rc = gnn::launch_scan_exclusive(a.csum + w * a.cstride, nch, a.coff + w * a.cstride, st);
    if (rc) return rc;
  }
  lw_chunk_add_kernel<<<dim3((unsigned)ceil_div(kcap + 1, 256), SG_SCANS), dim3(256), 0, st>>>(a);
  GNN_LAUNCHED("lw_chunk_add_kernel");
  return 0;
}

}  // extern "C"
