// step.hip — native executor of one GraphSAGE / GCN training step's forward + backward
// (include/gnn_step.h).
//
// Reference (main.py:122-146): output = model(x0, adjs, sampled_nodes); loss = utils.loss(...);
// loss.backward() — GraphSageConvolution / GraphConvolution (models.py:6-64) per layer, GNN's
// head (models.py:86-97) and the loss (utils.py:129-140: BCE with logits, or softmax cross-entropy
// for GNN_SH_LOSS_KIND = GNN_LOSS_CE), autograd for the backward.
//
// The Python path (gnn_amd.models fused=True) already runs every piece as a hand-written HIP
// kernel, but through ~45 autograd Functions and ctypes calls per step: 1.2-1.5 ms of host time
// against a 1.8 ms GPU step. This executor issues the same kernel sequence from C++ — one
// call per step, every intermediate carved from one caller-provided workspace — with the same
// numerics: the same kernels with the same arguments and routing (the split3 GEMM where its
// tiles fill the chip, the vendor GEMM (rocBLAS) for the small products), the same dropout
// seeds. Only the two products torch would run through its own reduction (the head's bias
// gradient, a column sum) use a fixed-order kernel here.
//
// Sequence (L layers, bottom-up index l; layer 0's input is the features, so it has no input
// gradient):
//   forward  l = 0..L-1:  feat = A_l·X (gnn_spmm_csr_f32; layer 0 over 16-bit X0 rows, GNN_SL_XKIND:
//                         gnn_spmm_csr_h16_f32);  [SAGE] xs = X[sampled] (row gather; widening there)
//                         [hB,] hW = [xs, feat]·[W_B, W_W]ᵀ  (one batched split3 launch or rocBLAS)
//                         Y_l = sage_norm(hB + b_B, hW + b_W)  (ELU, row standardise, scale/offset, dropout)
//   head:                 loss, z = BCE or CE(linear(dropout(normalize(Y_{L-1}))))
//   backward head:        dz, dY_{L-1};  dW_h = dzᵀ·xd (rocBLAS), db_h = colsum(dz)
//   backward l = L-1..0:  dhB, dhW, dscale, doffset, dbB, dbW = sage_norm_bwd(dY_l)
//                         dW_B, dW_W = [dhB, dhW]ᵀ·[xs, feat]  (split-k split3 from 2048 rows)
//                         l >= 1: dxs, dfeat = [dhB, dhW]·[W_B, W_W];
//                                 dY_{l-1} = A_lᵀ·dfeat (+ dxs scattered through rmap, SAGE)
//   an order-0 layer (GNN_SL_DENSE, models.py:21, 59-60) has no operand:
//   forward:              hW = X·W_Wᵀ (X in place);  Y_l = sage_norm(hW + b_W), width N
//   backward:             dhW, dscale, doffset, dbW = sage_norm_bwd(dY_l);  dW_W = dhWᵀ·X;
//                         l >= 1: dY_{l-1} = dhW·W_W, written straight into that buffer
//
// gnn_eval_step_f32 (validation / test batches, main.py:178-199, 217-241) is the forward above
// with training = 0 — forward() below, called by both entry points — followed by the evaluation
// head (gnn_head_eval_loss_f32: loss, logits, per-class prediction counts), on a plan without
// backward buffers.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>

#include "common.h"
#include "gnn_layers.h"
#include "gnn_spmm.h"
#include "gnn_step.h"

namespace {

using gnn::align_up;
using gnn::ceil_div;

// db = Σ_rows dz (M x C, row-major): one workgroup per column, each thread a strided set of
// rows, then a fixed-order tree (deterministic). A thread per column summing all M rows in a
// dependent chain took ~48 us for 512 x 41.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ dz, int M, int C,
                                                     float* __restrict__ out) {
  __shared__ float red[4];
  const int c = blockIdx.x;
  float s = 0.0f;
  for (int r = threadIdx.x; r < M; r += 256) s += dz[(int64_t)r * C + c];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[c] = (red[0] + red[1]) + (red[2] + red[3]);
}

// A bump allocator over the workspace; with base == nullptr it only measures.
struct Arena {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(int64_t count) {
    const size_t bytes = align_up((size_t)(count > 0 ? count : 1) * sizeof(T), 256);
    T* p = base ? (T*)(base + off) : nullptr;
    off += bytes;
    return p;
  }
};

int64_t L(const int64_t* d, int l, int f) { return d[GNN_STEP_HEADER + l * GNN_STEP_LAYER_SLOTS + f]; }
template <typename T>
T* P(const int64_t* d, int l, int f) {
  return (T*)(uintptr_t)L(d, l, f);
}
template <typename T>
T* HP(const int64_t* d, int f) {
  return (T*)(uintptr_t)d[f];
}

// The split3 GEMM takes an unsplit product when its 128 x 128 tiles cover the CUs
// (gnn_amd/fused.py _mfma_fills) and every operand meets its contract (_gemm_ok).
bool fills(int64_t M, int64_t N, int n) { return ceil_div(M, 128) * ceil_div(N, 128) * n >= 256; }
bool gemm_ok(const void* p, int64_t ld) { return ((uintptr_t)p % 8) == 0 && (ld % 2) == 0; }

std::mutex g_blas_mu;
rocblas_handle g_blas[64][2] = {};

// which = 0: the step's stream; 1: the aux stream (its own handle, so the two streams' small
// products never share a handle's workspace)
int blas_handle(rocblas_handle* h, int which = 0) {
  int dev = 0;
  GNN_HIP(hipGetDevice(&dev), "hipGetDevice");
  GNN_REQUIRE(dev >= 0 && dev < 64, "gnn_train_step: device index %d", dev);
  std::lock_guard<std::mutex> g(g_blas_mu);
  if (!g_blas[dev][which]) {
    if (rocblas_create_handle(&g_blas[dev][which]) != rocblas_status_success)
      return gnn::fail(-1, "rocblas_create_handle failed");
  }
  *h = g_blas[dev][which];
  return 0;
}

// The aux stream of a (device, priority): the work of a layer that does not depend on its
// aggregation — the x[sampled] gather and its GEMM in the forward, the weight-gradient GEMMs in
// the backward — can run there, beside the L2-gather-bound SpMM on the caller's stream. Forked and joined with events from a small
// per-stream pool; the pool's mutex is held for the whole step (events are re-recorded per call).
struct Aux {
  hipStream_t s = nullptr;
  hipEvent_t ev[24] = {};
  int next = 0;
  std::mutex mu;
  hipEvent_t take() { return ev[next++ % 24]; }
};
std::mutex g_aux_mu;
Aux* g_aux[64][4] = {};

int aux_of(hipStream_t st, Aux** out) {
  int dev = 0;
  GNN_HIP(hipGetDevice(&dev), "hipGetDevice");
  GNN_REQUIRE(dev >= 0 && dev < 64, "gnn_train_step: device index %d", dev);
  int prio = 0, lo = 0, hi = 0;
  GNN_HIP(hipStreamGetPriority(st, &prio), "hipStreamGetPriority");
  GNN_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi), "hipDeviceGetStreamPriorityRange");
  const int slot = std::min(3, std::max(0, lo - prio));  // lo = least urgent
  std::lock_guard<std::mutex> g(g_aux_mu);
  Aux*& a = g_aux[dev][slot];
  if (!a) {
    std::unique_ptr<Aux> n(new Aux());
    GNN_HIP(hipStreamCreateWithPriority(&n->s, hipStreamNonBlocking, prio), "hipStreamCreateWithPriority");
    for (auto& e : n->ev) GNN_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreateWithFlags");
    a = n.release();
  }
  *out = a;
  return 0;
}

// `to` waits for everything issued so far on `from`
int fork_join(Aux* a, hipStream_t from, hipStream_t to) {
  hipEvent_t e = a->take();
  GNN_HIP(hipEventRecord(e, from), "hipEventRecord");
  GNN_HIP(hipStreamWaitEvent(to, e, 0), "hipStreamWaitEvent");
  return 0;
}

// GNN_STEP_GATHER=1: gather x[sampled] first even where the GEMMs could read it in place (A/B)
bool no_index() {
  // read per call, as f32_gemm() below (bench.py's `gemm_ab` pass toggles GNN_GEMM_ALGO)
  const char* e = getenv("GNN_STEP_GATHER");
  const char* a = getenv("GNN_GEMM_ALGO");
  return (e && atoi(e) != 0) || (a && std::string(a) == "f32");  // the f32 kernel has no indexed form
}

// GNN_GEMM_ALGO=f32: the layer GEMMs on the f32-input MFMA kernel (gnn_gemm_f32, exact fp32)
// instead of split3 — the same routing, x[sampled] gathered (no row-indexed operands), no aux
// stream. For the end-to-end A/B of the two kernels (gnn_amd.fused reads the same variable).
bool f32_gemm() {
  const char* e = getenv("GNN_GEMM_ALGO");  // read per call (bench.py's `gemm_ab` pass toggles it)
  return e && std::string(e) == "f32";
}

// The split kernel's piece count for a layer whose GNN_SL_GEMM slot is np: the slot's, or for 0 what
// GNN_GEMM_ALGO says (split2: 2, bf16: 1 — the reduced-precision modes of gnn_gemm_f32_split,
// process-wide; anything else: split3). Read per call, as f32_gemm().
int pieces_of(int np) {
  if (np) return np;
  const char* e = getenv("GNN_GEMM_ALGO");
  if (!e) return 3;
  const std::string a(e);
  return a == "split2" ? 2 : a == "bf16" ? 1 : 3;
}

// np: the layer's GNN_SL_GEMM slot (0: GNN_GEMM_ALGO decides, f32 included)
int gemm(int np, int ak, int bk, int64_t M, int64_t N, int64_t K, int nb, const float* const* A, int64_t lda,
         const float* const* B, int64_t ldb, float* const* C, int64_t ldc, void* ws, size_t wsb, hipStream_t st) {
  if (np == 0 && f32_gemm()) return gnn_gemm_f32(ak, bk, M, N, K, nb, A, lda, B, ldb, C, ldc, ws, wsb, st);
  return gnn_gemm_f32_split(pieces_of(np), ak, bk, M, N, K, nb, A, lda, B, ldb, C, ldc, ws, wsb, st);
}

// (the reduced piece counts plan as split3 at its 128 x 128 tile: the same bytes unless
// GNN_GEMM_WIDE moves split3 itself to the wide tile)
size_t gemm_ws(int64_t M, int64_t N, int64_t K, int nb) {
  return std::max({gnn_gemm_f32_split3_workspace_bytes(M, N, K, nb), gnn_gemm_f32_workspace_bytes(M, N, K, nb),
                   gnn_gemm_f32_split_workspace_bytes(2, M, N, K, nb)});
}

// GNN_STEP_OVERLAP=1 turns the aux stream on. Off by default: measured on the Reddit config-2
// step it changed nothing (550 mini-batches/s either way; the layer-0/1 aggregations slowed from
// 239 to 261 us while the GEMMs ran beside them — the CUs are already saturated).
// GNN_STEP_FUSE_AGG=0: launch the top layer's backward aggregation on its own instead of folding
// it into the layer-1 tail backward (A/B; the values are bit-identical either way)
bool fuse_agg_enabled() {
  const char* e = getenv("GNN_STEP_FUSE_AGG");  // read per step (tests toggle it in-process)
  return !(e && atoi(e) == 0);
}

// GNN_STEP_SMALL_OVERLAP=0 keeps everything on the step's stream. By default the top layer's
// small, latency-bound pieces that do not depend on each other run on the aux stream: in the
// forward x[sampled] + linearB beside the aggregation + linearW; in the backward the head's and
// the top layer's weight gradients beside the input gradients and the layer below (same kernels,
// same handles' results: bit-identical).
bool small_overlap_enabled() {
  const char* e = getenv("GNN_STEP_SMALL_OVERLAP");
  return !(e && atoi(e) == 0);
}

bool overlap_enabled() {
  const char* e = getenv("GNN_STEP_OVERLAP");  // read per step (tests toggle it in-process)
  return e && atoi(e) != 0;
}

// Row-major products on rocBLAS (column-major underneath): the small layer-2 / head products.
int sgemm(rocblas_handle h, rocblas_operation ta, rocblas_operation tb, int64_t m, int64_t n, int64_t k,
          const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc) {
  const float one = 1.0f, zero = 0.0f;
  if (rocblas_sgemm(h, ta, tb, (rocblas_int)m, (rocblas_int)n, (rocblas_int)k, &one, A, (rocblas_int)lda, B,
                    (rocblas_int)ldb, &zero, C, (rocblas_int)ldc) != rocblas_status_success)
    return gnn::fail(-1, "rocblas_sgemm failed (m %lld n %lld k %lld)", (long long)m, (long long)n, (long long)k);
  return 0;
}
// out (M x N) = x (M x K) · Wᵀ (W: N x K)
int mm_xwt(rocblas_handle h, const float* x, int64_t ldx, const float* W, int64_t ldw, float* out, int64_t ldo,
           int64_t M, int64_t N, int64_t K) {
  return sgemm(h, rocblas_operation_transpose, rocblas_operation_none, N, M, K, W, ldw, x, ldx, out, ldo);
}
// out (M x K) = g (M x N) · W (N x K)
int mm_gw(rocblas_handle h, const float* g, int64_t ldg, const float* W, int64_t ldw, float* out, int64_t ldo,
          int64_t M, int64_t K, int64_t N) {
  return sgemm(h, rocblas_operation_none, rocblas_operation_none, K, M, N, W, ldw, g, ldg, out, ldo);
}
// out (N x K) = gᵀ (g: M x N) · x (M x K)
int mm_gtx(rocblas_handle h, const float* g, int64_t ldg, const float* x, int64_t ldx, float* out, int64_t ldo,
           int64_t N, int64_t K, int64_t M) {
  return sgemm(h, rocblas_operation_none, rocblas_operation_transpose, K, N, M, x, ldx, g, ldg, out, ldo);
}

// The per-layer buffers of one step (carved in a fixed order: sizing and running share it).
struct LayerBufs {
  int64_t M, K, nnz, F, Fk, ldx, ldo, N, D;
  bool xs_gathered;  // false: x[sampled] is read in place by the split3 GEMMs (row-indexed X)
  // an order-0 layer (GNN_SL_DENSE): no operand, Y = sage_norm(X·W_Wᵀ) of width D = N; X is read in
  // place (a 16-bit X0 widened once into feat, rows of ldo floats), and the input gradient dhW·W_W
  // is written straight into the layer below's dY
  bool dense;
  int np;  // GNN_SL_GEMM: pieces of the layer's split-kernel products (0: GNN_GEMM_ALGO, see pieces_of)
  const float* X;
  // layer 0 over a 16-bit X0 (GNN_SL_XKIND = GNN_FEAT_F16 / GNN_FEAT_BF16): X is NULL, X16 the rows
  // (ldx in elements); the aggregation reads them as they are and x[sampled] is widened into xs
  int xk;
  const void* X16;
  float *feat, *xs, *hB, *hW, *Y, *mean, *rstd;
  float *dY, *dhB, *dhW, *dxs, *dfeat;
  void *ws_fwd, *ws_bwd, *ws_norm, *ws_gemm_f, *ws_gemm_f2, *ws_gemm_dx, *ws_gemm_dw;
  size_t b_fwd, b_bwd, b_norm, b_gemm_f, b_gemm_dx, b_gemm_dw;
  // dY given as the aggregation of the layer above (its backward SpMM folded into this layer's
  // tail backward, gnn_sage_norm_bwd_agg_f32) instead of a dense buffer
  bool dy_agg;
  const int32_t *agg_rp, *agg_col, *agg_rmap;
  const float *agg_val, *agg_G, *agg_R;
  // the fp32 rows an order-0 layer's products read, and their stride
  const float* in() const { return xk ? feat : X; }
  int64_t ldin() const { return xk ? ldo : ldx; }
};

struct Plan {
  int nl = 0, sage = 1;
  LayerBufs lb[GNN_STEP_MAX_LAYERS];
  float *xd, *z, *nrm, *rowloss, *lse, *dz, *dXh;
  int loss_kind = GNN_LOSS_BCE;
  uint64_t* rowmask;  // the evaluation head's per-row class masks (gnn_head_eval_f32)
  int64_t Mh = 0, Dh = 0, C = 0;
};

#define GNN_TRY(x)        \
  do {                    \
    int rc_ = (x);        \
    if (rc_) return rc_;  \
  } while (0)

// The descriptor's shapes: what the layers' and the head's kernels are called with, no buffer
// yet (the training and the evaluation plan carve differently). measuring: X0 is taken as aligned.
int shapes(const int64_t* d, bool measuring, Plan& pl) {
  GNN_REQUIRE(d[GNN_SH_VERSION] == GNN_STEP_VERSION, "gnn_train_step: descriptor version %lld",
              (long long)d[GNN_SH_VERSION]);
  GNN_REQUIRE(d[GNN_SH_LOSS_KIND] == GNN_LOSS_BCE || d[GNN_SH_LOSS_KIND] == GNN_LOSS_CE,
              "gnn_train_step: loss kind %lld (0: BCE, 1: CE)", (long long)d[GNN_SH_LOSS_KIND]);
  pl.loss_kind = (int)d[GNN_SH_LOSS_KIND];
  pl.nl = (int)d[GNN_SH_LAYERS];
  pl.sage = d[GNN_SH_KIND] == GNN_STEP_SAGE;
  GNN_REQUIRE(pl.nl >= 1 && pl.nl <= GNN_STEP_MAX_LAYERS, "gnn_train_step: %d layers", pl.nl);
  const int64_t N = d[GNN_SH_NHID];
  const int n = pl.sage ? 2 : 1;
  for (int l = 0; l < pl.nl; ++l) {
    LayerBufs& b = pl.lb[l];
    b.dy_agg = false;
    b.M = L(d, l, GNN_SL_M);
    b.K = L(d, l, GNN_SL_K);
    b.nnz = L(d, l, GNN_SL_NNZ);
    b.N = N;
    const int64_t dense = L(d, l, GNN_SL_DENSE);
    GNN_REQUIRE(dense == 0 || dense == 1, "gnn_train_step: layer %d dense flag %lld (0: aggregating, 1: order 0)", l,
                (long long)dense);
    b.dense = dense != 0;
    const int64_t np = L(d, l, GNN_SL_GEMM);
    GNN_REQUIRE(np >= 0 && np <= 3,
                "gnn_train_step: layer %d GEMM pieces %lld (0: GNN_GEMM_ALGO, 1: bf16, 2: split2, 3: split3)", l,
                (long long)np);
    b.np = (int)np;
    b.D = b.dense ? N : n * N;
    if (b.dense) {
      GNN_REQUIRE(b.K == b.M, "gnn_train_step: order-0 layer %d has K = %lld, M = %lld", l, (long long)b.K,
                  (long long)b.M);
      b.nnz = 0;  // no operand: the slot is ignored
    }
    const int64_t xk = L(d, l, GNN_SL_XKIND);
    GNN_REQUIRE(xk == GNN_FEAT_F32 || (l == 0 && (xk == GNN_FEAT_F16 || xk == GNN_FEAT_BF16)),
                "gnn_train_step: layer %d input kind %lld (0: fp32; 1 fp16 / 2 bf16 on layer 0 only)", l,
                (long long)xk);
    b.xk = (int)xk;
    b.X16 = nullptr;
    if (l == 0) {
      b.X = xk ? nullptr : HP<const float>(d, GNN_SH_X0);
      b.X16 = xk ? HP<const void>(d, GNN_SH_X0) : nullptr;
      b.ldx = d[GNN_SH_LDX0];
      b.F = d[GNN_SH_F0];
    } else {
      const LayerBufs& p = pl.lb[l - 1];
      GNN_REQUIRE(b.K == p.M, "gnn_train_step: layer %d has K = %lld, layer %d M = %lld", l, (long long)b.K, l - 1,
                  (long long)p.M);
      b.X = nullptr;  // the layer below's output: a 256-byte aligned workspace buffer, set by the plan
      b.ldx = p.D;
      b.F = p.D;
    }
    GNN_REQUIRE(b.F <= b.ldx && b.F > 0 && b.M > 0 && b.K > 0, "gnn_train_step: layer %d shape", l);
    // the aggregation's padded width (custom_sparse_ops.spmm_csr): 16-byte loads over whole
    // line-aligned rows when the input rows are padded (the 602-wide features in 608-float rows)
    b.Fk = b.F;
    if (b.F % 4 && b.ldx % 4 == 0 && (l >= 1 || (uintptr_t)b.X % 16 == 0 || measuring) &&
        b.ldx >= b.F + (4 - b.F % 4))
      b.Fk = b.F + (4 - b.F % 4);
    b.ldo = (b.Fk != b.F && b.ldx <= 2 * b.Fk) ? b.ldx : b.Fk;
    if (xk) {
      // 16-bit rows: 4 elements per load and no narrower form (gnn_spmm_csr_h16_f32), so the padded
      // width must fit the row; the output takes the stride an fp32 X0 of this store has (whole
      // 128-byte lines), so the workspace is that of the widened step
      GNN_REQUIRE(b.ldx % 4 == 0 && ((uintptr_t)b.X16 % 8 == 0 || measuring),
                  "gnn_train_step: 16-bit x0 needs 8-byte aligned rows (ldx %lld)", (long long)b.ldx);
      b.Fk = (int64_t)align_up((size_t)b.F, 4);
      GNN_REQUIRE(b.Fk <= b.ldx, "gnn_train_step: 16-bit x0 rows of %lld elements have no room for %lld columns",
                  (long long)b.ldx, (long long)b.Fk);
      b.ldo = (int64_t)align_up((size_t)b.Fk, 32);
    }
    b.b_fwd = b.dense ? 0 : gnn_spmm_workspace_bytes(b.M, b.nnz, b.Fk, 0);
    b.b_gemm_f = gemm_ws(b.M, N, b.F, b.dense ? 1 : n);
  }
  const LayerBufs& top = pl.lb[pl.nl - 1];
  pl.Mh = top.M;
  pl.Dh = top.D;
  pl.C = d[GNN_SH_CLASSES];
  GNN_REQUIRE(pl.C > 0 && pl.C <= 256 && pl.Dh % 4 == 0 && pl.Dh <= 2048, "gnn_train_step: head %lld x %lld",
              (long long)pl.Dh, (long long)pl.C);
  return 0;
}

// The evaluation step's plan (gnn_eval_step_f32): no backward buffer, and ONE set of forward
// buffers for all layers (sized for the largest), the layer outputs in two that alternate. Safe
// with the forward's aux stream: each layer joins it before its tail, and the next layer forks
// it again from the step's stream, so no buffer is rewritten while the other stream may read it.
int plan_eval(const int64_t* d, Arena& ar, Plan& pl) {
  GNN_TRY(shapes(d, !ar.base, pl));
  int64_t feat = 0, xs = 0, h = 0, rows = 0, y[2] = {0, 0};
  size_t wf = 0, wg = 0;
  bool agg = false;  // any aggregating layer: feat, the SpMM workspace and (SAGE) xs, hB, the aux product
  for (int l = 0; l < pl.nl; ++l) {
    const LayerBufs& b = pl.lb[l];
    agg = agg || !b.dense;
    // an order-0 layer reads X in place: no feat (but the widened rows of a 16-bit X0)
    if (!b.dense || b.xk) feat = std::max(feat, b.M * b.ldo);
    if (!b.dense) xs = std::max(xs, b.M * b.ldo);
    h = std::max(h, b.M * b.N);
    rows = std::max(rows, b.M);
    y[l & 1] = std::max(y[l & 1], b.M * b.D);
    wf = std::max(wf, b.b_fwd);
    wg = std::max(wg, b.b_gemm_f);
  }
  LayerBufs s = {};
  const bool pair = pl.sage && agg;
  s.feat = (agg || feat) ? ar.take<float>(feat) : nullptr;
  s.xs = pair ? ar.take<float>(xs) : nullptr;
  s.hB = pair ? ar.take<float>(h) : nullptr;
  s.hW = ar.take<float>(h);
  float* const Y[2] = {ar.take<float>(y[0]), ar.take<float>(y[1])};
  s.mean = ar.take<float>(rows);
  s.rstd = ar.take<float>(rows);
  s.ws_fwd = agg ? ar.take<char>((int64_t)wf) : nullptr;
  s.ws_gemm_f = ar.take<char>((int64_t)wg);
  s.ws_gemm_f2 = pair ? ar.take<char>((int64_t)wg) : nullptr;
  for (int l = 0; l < pl.nl; ++l) {
    LayerBufs& b = pl.lb[l];
    if (l) b.X = pl.lb[l - 1].Y;
    b.feat = s.feat, b.xs = s.xs, b.hB = s.hB, b.hW = s.hW, b.Y = Y[l & 1], b.mean = s.mean, b.rstd = s.rstd;
    b.ws_fwd = s.ws_fwd, b.ws_gemm_f = s.ws_gemm_f, b.ws_gemm_f2 = s.ws_gemm_f2;
  }
  pl.rowloss = ar.take<float>(pl.Mh);
  pl.rowmask = ar.take<uint64_t>(pl.Mh * 8);
  return 0;
}

int plan(const int64_t* d, Arena& ar, Plan& pl) {
  GNN_TRY(shapes(d, !ar.base, pl));
  const int64_t N = d[GNN_SH_NHID];
  const int n = pl.sage ? 2 : 1;
  for (int l = 0; l < pl.nl; ++l) {
    LayerBufs& b = pl.lb[l];
    if (l) b.X = pl.lb[l - 1].Y;
    const bool pair = pl.sage && !b.dense;
    b.feat = (!b.dense || b.xk) ? ar.take<float>(b.M * b.ldo) : nullptr;
    b.xs = pair ? ar.take<float>(b.M * b.ldo) : nullptr;
    b.hB = pair ? ar.take<float>(b.M * N) : nullptr;
    b.hW = ar.take<float>(b.M * N);
    b.Y = ar.take<float>(b.M * b.D);
    b.mean = ar.take<float>(b.M);
    b.rstd = ar.take<float>(b.M);
    b.ws_fwd = b.dense ? nullptr : ar.take<char>((int64_t)b.b_fwd);
    b.ws_gemm_f = ar.take<char>((int64_t)b.b_gemm_f);
    b.ws_gemm_f2 = pair ? ar.take<char>((int64_t)b.b_gemm_f) : nullptr;  // the aux stream's product
  }
  pl.xd = ar.take<float>(pl.Mh * pl.Dh);
  pl.z = ar.take<float>(pl.Mh * pl.C);
  pl.nrm = ar.take<float>(pl.Mh);
  pl.rowloss = ar.take<float>(pl.Mh);
  pl.lse = ar.take<float>(pl.Mh);  // the rows' log-sum-exp (GNN_LOSS_CE)
  pl.dz = ar.take<float>(pl.Mh * pl.C);
  pl.dXh = ar.take<float>(pl.Mh * pl.Dh);
  for (int l = pl.nl - 1; l >= 0; --l) {
    LayerBufs& b = pl.lb[l];
    b.dY = (l == pl.nl - 1) ? pl.dXh : nullptr;  // set below for l < nl-1
    b.dhB = (pl.sage && !b.dense) ? ar.take<float>(b.M * N) : nullptr;
    b.dhW = ar.take<float>(b.M * N);
    b.b_norm = gnn_sage_norm_bwd_workspace_bytes(b.M, b.D);
    b.ws_norm = ar.take<char>((int64_t)b.b_norm);
    b.b_gemm_dw = gemm_ws(N, b.F, b.M, b.dense ? 1 : n);
    b.ws_gemm_dw = ar.take<char>((int64_t)b.b_gemm_dw);
    if (l >= 1 && b.dense) {
      // the input gradient dhW·W_W goes straight into layer l-1's dY: no dfeat / dxs, no SpMM
      b.dxs = b.dfeat = nullptr;
      b.b_gemm_dx = gemm_ws(b.M, b.F, N, 1);
      b.ws_gemm_dx = ar.take<char>((int64_t)b.b_gemm_dx);
      b.ws_bwd = nullptr;
      b.b_bwd = 0;
    } else if (l >= 1) {
      b.dxs = pl.sage ? ar.take<float>(b.M * b.F) : nullptr;
      b.dfeat = ar.take<float>(b.M * b.F);
      b.b_gemm_dx = gemm_ws(b.M, b.F, N, n);
      b.ws_gemm_dx = ar.take<char>((int64_t)b.b_gemm_dx);
      b.b_bwd = gnn_spmm_workspace_bytes(b.K, b.nnz, b.F, 0);
      b.ws_bwd = ar.take<char>((int64_t)b.b_bwd);
    } else {
      b.dxs = b.dfeat = nullptr;
      b.ws_gemm_dx = b.ws_bwd = nullptr;
      b.b_gemm_dx = b.b_bwd = 0;
    }
  }
  // dY of layer l < nl-1 is the input gradient of layer l+1 (K_{l+1} x F_{l+1} = M_l x D_l)
  for (int l = 0; l < pl.nl - 1; ++l) pl.lb[l].dY = ar.take<float>(pl.lb[l].M * pl.lb[l].D);
  return 0;
}

// What one call holds while it issues its kernels: the plan, the streams, the vendor-GEMM handles
// (held with the aux stream's lock), and the descriptor's optional hooks.
struct Run {
  const int64_t* d = nullptr;
  Plan pl;
  hipStream_t st = nullptr;
  rocblas_handle h = nullptr, ha = nullptr;  // ha: the aux stream's handle (small products there)
  Aux* aux = nullptr;
  std::unique_lock<std::mutex> aux_lock;
  bool big_ov = false;  // the big layers' GEMMs beside their SpMMs (off)
  float p = 0.0f;
  int training = 0;
  int64_t phase = 0;
  int64_t* T = nullptr;  // per-aggregation timing records (GNN_SH_TIMING)
  int64_t nrec = 0;

  int open(const int64_t* desc, hipStream_t stream) {
    d = desc;
    st = stream;
    GNN_TRY(blas_handle(&h));
    if (rocblas_set_stream(h, st) != rocblas_status_success) return gnn::fail(-1, "rocblas_set_stream failed");
    const int32_t bits = (int32_t)d[GNN_SH_PDROP_BITS];
    std::memcpy(&p, &bits, 4);
    big_ov = overlap_enabled() && !f32_gemm();
    const bool small_ov = small_overlap_enabled();
    if (big_ov || small_ov) GNN_TRY(aux_of(st, &aux));
    if (aux) aux_lock = std::unique_lock<std::mutex>(aux->mu);
    if (aux && small_ov) {
      GNN_TRY(blas_handle(&ha, 1));
      if (rocblas_set_stream(ha, aux->s) != rocblas_status_success) return gnn::fail(-1, "rocblas_set_stream failed");
    }
    return 0;
  }
  // optional per-aggregation timing (GNN_SH_TIMING): arm the caller's event pair for the next
  // SpMM launch (gnn_spmm_set_timing_events) and record the call's shape beside it
  void arm(int64_t kind, int64_t l, int64_t M, int64_t K, int64_t nnz, int64_t F, int64_t Fk, int64_t ldx,
           int64_t ldo, const void* X, const void* Y, int64_t res_rows, int64_t xkind = 0) {
    if (!T || nrec >= T[0]) return;
    int64_t* r = T + 1 + GNN_STEP_TIMING_SLOTS * nrec++;
    gnn_spmm_set_timing_events((void*)r[0], (void*)r[1]);
    const int64_t v[] = {kind, l, M, K, nnz, F, Fk, ldx, ldo, (int64_t)(uintptr_t)X, (int64_t)(uintptr_t)Y, res_rows, 1,
                         xkind};
    std::memcpy(r + 2, v, sizeof v);
  }
  // layer l's forward aggregation feat = A_l·X (armed for timing), over fp32 or 16-bit rows
  int aggregate(int l) {
    const LayerBufs& b = pl.lb[l];
    arm(0, l, b.M, b.K, b.nnz, b.F, b.Fk, b.ldx, b.ldo, b.xk ? b.X16 : (const void*)b.X, b.feat, 0, b.xk);
    const int32_t* rp = P<const int32_t>(d, l, GNN_SL_ROWPTR);
    const int32_t* col = P<const int32_t>(d, l, GNN_SL_COL);
    const float* val = P<const float>(d, l, GNN_SL_VAL);
    if (b.xk)
      return gnn_spmm_csr_h16_f32(rp, col, val, b.M, b.K, b.nnz, b.X16, b.ldx, b.xk, b.feat, b.ldo, b.Fk, b.ws_fwd,
                                  b.b_fwd, 0, st);
    return gnn_spmm_csr_f32(rp, col, val, b.M, b.K, b.nnz, b.X, b.ldx, b.feat, b.ldo, b.Fk, b.ws_fwd, b.b_fwd, 0, st);
  }
  // xs = X[sampled] on stream s (16-bit rows widen on the way: exact)
  int gather_sampled(int l, hipStream_t s) {
    const LayerBufs& b = pl.lb[l];
    const int64_t* idx = P<const int64_t>(d, l, GNN_SL_SAMPLED);
    if (b.xk) return gnn_gather_rows_h16_f32(b.X16, b.ldx, b.xk, idx, b.xs, b.ldo, nullptr, b.M, b.F, s);
    return gnn_gather_rows_f32(b.X, b.ldx, idx, b.xs, b.ldo, nullptr, b.M, b.F, s);
  }
  // the staging gate (GNN_SH_STAGE_EVENT): recorded right after the chosen layer's forward
  // aggregation is issued; for an order-0 layer where that aggregation would have been, before
  // the layer's GEMM
  int stage_gate(int l) {
    if (d[GNN_SH_STAGE_EVENT] && l == (int)d[GNN_SH_STAGE_LAYER])
      GNN_HIP(hipEventRecord((hipEvent_t)d[GNN_SH_STAGE_EVENT], st), "hipEventRecord (stage gate)");
    return 0;
  }
};

// The layers' forward, bottom-up, into the plan's buffers: shared by the training step and the
// evaluation step (training = 0), so both issue the same kernels with the same routing.
int forward(Run& r) {
  const int64_t* const d = r.d;
  Plan& pl = r.pl;
  hipStream_t st = r.st;
  rocblas_handle h = r.h, ha = r.ha;
  Aux* aux = r.aux;
  const bool big_ov = r.big_ov;
  const int64_t phase = r.phase;
  const int n = pl.sage ? 2 : 1;
  for (int l = 0; l < pl.nl; ++l) {
    LayerBufs& b = pl.lb[l];
    const int64_t N = b.N;
    const float* WB = P<const float>(d, l, GNN_SL_WB);
    const float* WW = P<const float>(d, l, GNN_SL_WW);
    if (b.dense) {
      // order 0 (models.py:21, 59-60): hW = X·W_Wᵀ with X read in place, one product routed as
      // the pairs below; then the tail in its D1 = 0 form. No operand, no x[sampled], no aux stream.
      if (phase != 2 || l != 0) GNN_TRY(r.stage_gate(l));  // where the aggregation would have been
      if (b.xk)  // 16-bit X0: widened once (exact), then the layer runs as fp32
        GNN_TRY(gnn_gather_rows_h16_f32(b.X16, b.ldx, b.xk, nullptr, b.feat, b.ldo, nullptr, b.M, b.F, st));
      const float* X = b.in();
      const int64_t ldx = b.ldin();
      b.xs_gathered = true;
      if (gemm_ok(X, ldx) && gemm_ok(WW, b.F) && fills(b.M, N, 1)) {
        const float* A[1] = {X};
        const float* B[1] = {WW};
        float* Cc[1] = {b.hW};
        GNN_TRY(gemm(b.np, 0, 0, b.M, N, b.F, 1, A, ldx, B, b.F, Cc, N, b.ws_gemm_f, b.b_gemm_f, st));
      } else {
        GNN_TRY(mm_xwt(h, X, ldx, WW, b.F, b.hW, N, b.M, N, b.F));
      }
      GNN_TRY(gnn_sage_norm_fwd_f32(nullptr, 4, 0, b.hW, N, N, nullptr, P<const float>(d, l, GNN_SL_BW),
                                    P<const float>(d, l, GNN_SL_SCALE), P<const float>(d, l, GNN_SL_OFFSET), b.M, r.p,
                                    (uint64_t)L(d, l, GNN_SL_SEED), r.training, b.Y, b.D, b.mean, b.rstd, st));
      continue;
    }
    if (pl.sage)
      GNN_REQUIRE(L(d, l, GNN_SL_NSAMPLED) == b.M, "gnn_train_step: layer %d sampled %lld != M %lld", l,
                  (long long)L(d, l, GNN_SL_NSAMPLED), (long long)b.M);
    const bool ok = gemm_ok(b.feat, b.ldo) && gemm_ok(WW, b.F) && (!pl.sage || gemm_ok(WB, b.F));
    // the top layer's small products (rocBLAS): x[sampled] + linearB on the aux stream beside A·X
    const bool small_side = ha && pl.sage && !(ok && fills(b.M, N, n));
    if (big_ov && pl.sage && ok && fills(b.M, N, n)) {
      // x[sampled] and linearB on the aux stream beside A·X and linearW; each product launched
      // alone with the split choice of the pair, so the sums are those of the batched launch
      b.xs_gathered = true;
      GNN_TRY(fork_join(aux, st, aux->s));
      GNN_TRY(r.gather_sampled(l, aux->s));
      const float* Ab[1] = {b.xs};
      const float* Bb[1] = {WB};
      float* Cb[1] = {b.hB};
      GNN_TRY(gnn::gemm_split3_as_batch(0, 0, b.M, N, b.F, 1, 2, 0, Ab, b.ldo, Bb, b.F, Cb, N, b.ws_gemm_f2, b.b_gemm_f,
                                        aux->s, pieces_of(b.np)));
      if (phase != 2 || l != 0) {
        GNN_TRY(r.aggregate(l));
        GNN_TRY(r.stage_gate(l));
      }
      const float* Aw[1] = {b.feat};
      const float* Bw[1] = {WW};
      float* Cw[1] = {b.hW};
      GNN_TRY(gnn::gemm_split3_as_batch(0, 0, b.M, N, b.F, 1, 2, 1, Aw, b.ldo, Bw, b.F, Cw, N, b.ws_gemm_f, b.b_gemm_f, st,
                                        pieces_of(b.np)));
      GNN_TRY(fork_join(aux, aux->s, st));
    } else if (small_side) {
      b.xs_gathered = true;
      GNN_TRY(fork_join(aux, st, aux->s));  // aux sees X complete
      GNN_TRY(r.gather_sampled(l, aux->s));
      GNN_TRY(mm_xwt(ha, b.xs, b.ldo, WB, b.F, b.hB, N, b.M, N, b.F));
      if (phase != 2 || l != 0) {
        GNN_TRY(r.aggregate(l));
        GNN_TRY(r.stage_gate(l));
      }
      GNN_TRY(mm_xwt(h, b.feat, b.ldo, WW, b.F, b.hW, N, b.M, N, b.F));
      GNN_TRY(fork_join(aux, aux->s, st));  // the tail reads hB
    } else {
      if (phase != 2 || l != 0) {
        GNN_TRY(r.aggregate(l));
        GNN_TRY(r.stage_gate(l));
      }
      // x[sampled] feeds only linearB and its weight gradient: when both run on split3 (and X's
      // rows have the aggregation output's stride) the GEMMs read X's rows through the index
      // instead of a gathered copy (bit-identical operands)
      // (16-bit X0 rows are always gathered, and widened on the way: the split3 GEMMs read fp32)
      b.xs_gathered =
          !(pl.sage && ok && fills(b.M, N, n) && b.M >= 2048 && b.ldx == b.ldo && !no_index() && !b.xk);
      if (pl.sage && b.xs_gathered) GNN_TRY(r.gather_sampled(l, st));
    }
    if ((big_ov && pl.sage && ok && fills(b.M, N, n)) || small_side) {
      // done above
    } else if (ok && fills(b.M, N, n) && !b.xs_gathered) {
      const float* A[2] = {b.X, b.feat};
      const int64_t* IA[2] = {P<const int64_t>(d, l, GNN_SL_SAMPLED), nullptr};
      const float* B[2] = {WB, WW};
      float* Cc[2] = {b.hB, b.hW};
      GNN_TRY(gnn::gemm_split3_indexed(0, 0, b.M, N, b.F, n, A, b.ldo, IA, b.K, B, b.F, nullptr, 0, Cc, N,
                                       b.ws_gemm_f, b.b_gemm_f, st, pieces_of(b.np)));
    } else if (ok && fills(b.M, N, n)) {
      const float* A[2] = {pl.sage ? b.xs : b.feat, b.feat};
      const float* B[2] = {pl.sage ? WB : WW, WW};
      float* Cc[2] = {pl.sage ? b.hB : b.hW, b.hW};
      GNN_TRY(gemm(b.np, 0, 0, b.M, N, b.F, n, A + (pl.sage ? 0 : 1), b.ldo, B + (pl.sage ? 0 : 1), b.F,
                   Cc + (pl.sage ? 0 : 1), N, b.ws_gemm_f, b.b_gemm_f, st));
    } else {
      if (pl.sage) GNN_TRY(mm_xwt(h, b.xs, b.ldo, WB, b.F, b.hB, N, b.M, N, b.F));
      GNN_TRY(mm_xwt(h, b.feat, b.ldo, WW, b.F, b.hW, N, b.M, N, b.F));
    }
    GNN_TRY(gnn_sage_norm_fwd_f32(pl.sage ? b.hB : nullptr, pl.sage ? N : 4, pl.sage ? N : 0, b.hW, N, N,
                                  pl.sage ? P<const float>(d, l, GNN_SL_BB) : nullptr, P<const float>(d, l, GNN_SL_BW),
                                  P<const float>(d, l, GNN_SL_SCALE), P<const float>(d, l, GNN_SL_OFFSET), b.M, r.p,
                                  (uint64_t)L(d, l, GNN_SL_SEED), r.training, b.Y, b.D, b.mean, b.rstd, st));
  }
  return 0;
}

// The workspace is validated before anything is launched: large enough for the plan, aligned.
int check_workspace(const void* workspace, size_t workspace_bytes, size_t need) {
  GNN_REQUIRE(workspace && workspace_bytes >= need, "gnn_train_step: workspace too small (%zu < %zu)",
              workspace_bytes, need);
  GNN_REQUIRE((uintptr_t)workspace % 256 == 0, "gnn_train_step: workspace not 256-byte aligned");
  return 0;
}

}  // namespace

extern "C" {

int gnn_head_bias_grad_f32(const float* dz, int64_t M, int64_t C, float* db, void* stream) {
  GNN_REQUIRE(M >= 0 && C >= 0 && M < INT_MAX && C < INT_MAX, "gnn_head_bias_grad_f32: bad size");
  if (C == 0) return 0;
  GNN_REQUIRE(db && (M == 0 || dz), "gnn_head_bias_grad_f32: NULL pointer");
  colsum_kernel<<<dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream>>>(dz, (int)M, (int)C, db);
  GNN_LAUNCHED("colsum_kernel");
  return 0;
}

size_t gnn_train_step_workspace_bytes(const int64_t* desc) {
  if (!desc) return 0;
  Arena ar{nullptr};
  Plan pl;
  if (plan(desc, ar, pl)) return 0;
  return ar.off;
}

int gnn_train_step_f32(const int64_t* d, void* workspace, size_t workspace_bytes, void* stream) {
  GNN_REQUIRE(d != nullptr, "gnn_train_step: NULL descriptor");
  Arena ar{(char*)workspace};
  Run r;
  Plan& pl = r.pl;
  {
    Arena dry{nullptr};
    Plan tmp;
    GNN_TRY(plan(d, dry, tmp));
    GNN_TRY(check_workspace(workspace, workspace_bytes, dry.off));
  }
  GNN_TRY(plan(d, ar, pl));
  hipStream_t st = (hipStream_t)stream;
  GNN_TRY(r.open(d, st));
  rocblas_handle h = r.h, ha = r.ha;
  Aux* aux = r.aux;
  const bool big_ov = r.big_ov;
  const int n = pl.sage ? 2 : 1;
  const float p = r.p;
  const int training = r.training = (int)d[GNN_SH_TRAINING];
  bool aux_used = false;
  r.T = HP<int64_t>(d, GNN_SH_TIMING);
  // phase (GNN_SH_PHASE): 1 = only layer 0's forward aggregation, into this workspace (a data-
  // parallel caller issues the next batch's while the gradient all-reduce runs); 2 = the step with
  // that aggregation already issued into this workspace by a phase-1 call (same descriptor plan)
  const int64_t phase = r.phase = d[GNN_SH_PHASE];
  GNN_REQUIRE(phase >= 0 && phase <= 2, "gnn_train_step: phase %lld", (long long)phase);
  if (phase == 1) {
    r.T = nullptr;  // the prefetched aggregation is not timed
    // an order-0 layer 0 has no aggregation to issue ahead: no kernel, only the gate if it is layer 0's
    if (!pl.lb[0].dense) GNN_TRY(r.aggregate(0));
    return r.stage_gate(0);
  }
  // ------------------------------------------------------------------ forward
  GNN_TRY(forward(r));
  // ------------------------------------------------------------------ head + loss
  const LayerBufs& top = pl.lb[pl.nl - 1];
  const float* Wh = HP<const float>(d, GNN_SH_HEAD_W);
  const uint64_t hseed = (uint64_t)d[GNN_SH_HEAD_SEED];
  const float* labels = HP<const float>(d, GNN_SH_LABELS);
  const int64_t ldl = d[GNN_SH_LDL];
  const bool ce = pl.loss_kind == GNN_LOSS_CE;
  if (ce)
    GNN_TRY(gnn_head_ce_fwd_f32(top.Y, top.D, pl.Mh, pl.Dh, Wh, HP<const float>(d, GNN_SH_HEAD_B), pl.C, labels, ldl, p,
                                hseed, training, pl.xd, pl.z, pl.nrm, pl.rowloss, HP<float>(d, GNN_SH_LOSS), pl.lse,
                                st));
  else
    GNN_TRY(gnn_head_bce_fwd_f32(top.Y, top.D, pl.Mh, pl.Dh, Wh, HP<const float>(d, GNN_SH_HEAD_B), pl.C, labels, ldl,
                                 p, hseed, training, pl.xd, pl.z, pl.nrm, pl.rowloss, HP<float>(d, GNN_SH_LOSS), st));
  // ------------------------------------------------------------------ backward
  if (ce)
    GNN_TRY(gnn_head_ce_bwd_f32(top.Y, top.D, pl.Mh, pl.Dh, Wh, pl.C, labels, ldl, nullptr, p, hseed, training, pl.z,
                                pl.nrm, pl.dz, pl.dXh, pl.Dh, pl.lse, st));
  else
    GNN_TRY(gnn_head_bce_bwd_f32(top.Y, top.D, pl.Mh, pl.Dh, Wh, pl.C, labels, ldl, nullptr, p, hseed, training, pl.z,
                                 pl.nrm, pl.dz, pl.dXh, pl.Dh, st));
  // gradient-ready events (GNN_SH_GRAD_EVENTS): the caller's DP exchange of a bucket starts there
  const int64_t* const E = HP<const int64_t>(d, GNN_SH_GRAD_EVENTS);
  auto grads_ready = [&](int64_t slot, hipStream_t s) -> int {
    if (E && slot < E[0] && E[slot]) GNN_HIP(hipEventRecord((hipEvent_t)E[slot], s), "hipEventRecord (grad event)");
    return 0;
  };
  // the head's weight and bias gradients (their inputs are final here). With the aux stream they
  // go there with the first small weight-gradient products of the backward below, behind the same
  // fork: every event recorded on or awaited by the step's stream costs it a ~7 us bubble between
  // kernels (profiles/round4/trace/), so the backward forks once, not twice.
  bool head_pending = true;
  auto head_grads = [&](hipStream_t s, rocblas_handle hh) -> int {
    GNN_TRY(mm_gtx(hh, pl.dz, pl.C, pl.xd, pl.Dh, HP<float>(d, GNN_SH_HEAD_GW), pl.Dh, pl.C, pl.Dh, pl.Mh));
    if (HP<float>(d, GNN_SH_HEAD_GB)) {
      colsum_kernel<<<dim3((unsigned)pl.C), dim3(256), 0, s>>>(pl.dz, (int)pl.Mh, (int)pl.C,
                                                             HP<float>(d, GNN_SH_HEAD_GB));
      GNN_LAUNCHED("colsum_kernel");
    }
    GNN_TRY(grads_ready(1, s));
    head_pending = false;
    return 0;
  };
  if (!ha) GNN_TRY(head_grads(st, h));
  for (int l = pl.nl - 1; l >= 0; --l) {
    LayerBufs& b = pl.lb[l];
    const int64_t N = b.N;
    const float* WB = P<const float>(d, l, GNN_SL_WB);
    const float* WW = P<const float>(d, l, GNN_SL_WW);
    const bool pair = pl.sage && !b.dense;  // an order-0 layer's tail is the D1 = 0 form
    if (b.dy_agg)  // the layer above's backward aggregation, computed as this tail reads its rows
      GNN_TRY(gnn_sage_norm_bwd_agg_f32(b.agg_rp, b.agg_col, b.agg_val, b.agg_G, b.D, b.agg_R, b.D, b.agg_rmap,
                                        pair ? b.hB : nullptr, pair ? N : 4, pair ? N : 0, b.hW, N, N,
                                        pair ? P<const float>(d, l, GNN_SL_BB) : nullptr,
                                        P<const float>(d, l, GNN_SL_BW), P<const float>(d, l, GNN_SL_SCALE), b.mean,
                                        b.rstd, b.M, p, (uint64_t)L(d, l, GNN_SL_SEED), training, b.dhB, b.dhW,
                                        P<float>(d, l, GNN_SL_GSCALE), P<float>(d, l, GNN_SL_GOFFSET),
                                        pair ? P<float>(d, l, GNN_SL_GBB) : nullptr, P<float>(d, l, GNN_SL_GBW),
                                        b.ws_norm, b.b_norm, st));
    else
      GNN_TRY(gnn_sage_norm_bwd_f32(b.dY, b.D, pair ? b.hB : nullptr, pair ? N : 4, pair ? N : 0, b.hW, N, N,
                                    pair ? P<const float>(d, l, GNN_SL_BB) : nullptr, P<const float>(d, l, GNN_SL_BW),
                                    P<const float>(d, l, GNN_SL_SCALE), b.mean, b.rstd, b.M, p,
                                    (uint64_t)L(d, l, GNN_SL_SEED), training, b.dhB, b.dhW,
                                    P<float>(d, l, GNN_SL_GSCALE), P<float>(d, l, GNN_SL_GOFFSET),
                                    pair ? P<float>(d, l, GNN_SL_GBB) : nullptr, P<float>(d, l, GNN_SL_GBW),
                                    b.ws_norm, b.b_norm, st));
    if (b.dense) {
      // order 0: the input gradient is a GEMM, written straight into layer l-1's dY (M x F, stride
      // F = D_{l-1}: no dfeat, no transpose, no SpMM, so nothing to fold below); the weight
      // gradient dhWᵀ·X reads X in place. Routed as the aggregating layers' products.
      const float* X = b.in();
      const int64_t ldx = b.ldin();
      const bool okd = gemm_ok(X, ldx) && gemm_ok(WW, b.F);
      const float* Gd[1] = {b.dhW};
      if (l >= 1) {
        float* dYp = pl.lb[l - 1].dY;
        if (okd && fills(b.M, b.F, 1)) {
          const float* B[1] = {WW};
          float* Cc[1] = {dYp};
          GNN_TRY(gemm(b.np, 0, 1, b.M, b.F, N, 1, Gd, N, B, b.F, Cc, b.F, b.ws_gemm_dx, b.b_gemm_dx, st));
        } else {
          GNN_TRY(mm_gw(h, b.dhW, N, WW, b.F, dYp, b.F, b.M, b.F, N));
        }
      }
      float* gWW = P<float>(d, l, GNN_SL_GWW);
      hipStream_t sw = st;
      if (okd && b.M >= 2048) {
        if (big_ov && l >= 1) {
          GNN_TRY(fork_join(aux, st, aux->s));
          sw = aux->s;
          aux_used = true;
        }
        const float* Xd[1] = {X};
        float* Cc[1] = {gWW};
        GNN_TRY(gemm(b.np, 1, 1, N, b.F, b.M, 1, Gd, N, Xd, ldx, Cc, b.F, b.ws_gemm_dw, b.b_gemm_dw, sw));
      } else {
        rocblas_handle hw = h;
        if (ha) {
          GNN_TRY(fork_join(aux, st, aux->s));
          sw = aux->s;
          hw = ha;
          aux_used = true;
          if (head_pending) GNN_TRY(head_grads(aux->s, ha));
        }
        GNN_TRY(mm_gtx(hw, b.dhW, N, X, ldx, gWW, b.F, N, b.F, b.M));
      }
      GNN_TRY(grads_ready(2 + l, sw));
      continue;
    }
    const bool ok = gemm_ok(b.feat, b.ldo) && gemm_ok(WW, b.F) && (!pl.sage || gemm_ok(WB, b.F));
    const float* G[2] = {pl.sage ? b.dhB : b.dhW, b.dhW};
    const int o = pl.sage ? 0 : 1;
    if (l >= 1) {  // input gradients (layer 0's input is the features)
      if (ok && fills(b.M, b.F, n)) {
        const float* B[2] = {pl.sage ? WB : WW, WW};
        float* Cc[2] = {pl.sage ? b.dxs : b.dfeat, b.dfeat};
        GNN_TRY(gemm(b.np, 0, 1, b.M, b.F, N, n, G + o, N, B + o, b.F, Cc + o, b.F, b.ws_gemm_dx, b.b_gemm_dx, st));
      } else {
        if (pl.sage) GNN_TRY(mm_gw(h, b.dhB, N, WB, b.F, b.dxs, b.F, b.M, b.F, N));
        GNN_TRY(mm_gw(h, b.dhW, N, WW, b.F, b.dfeat, b.F, b.M, b.F, N));
      }
    }
    // weight gradients: split over the sampled rows on split3 from 2048 rows, else rocBLAS; on
    // the aux stream (joined at the end of the step) beside the input-gradient GEMM + A_lᵀ·dfeat
    float* gWB = pl.sage ? P<float>(d, l, GNN_SL_GWB) : nullptr;
    float* gWW = P<float>(d, l, GNN_SL_GWW);
    if (ok && b.M >= 2048) {
      const float* X[2] = {pl.sage ? (b.xs_gathered ? b.xs : b.X) : b.feat, b.feat};
      const int64_t* IB[2] = {pl.sage && !b.xs_gathered ? P<const int64_t>(d, l, GNN_SL_SAMPLED) : nullptr, nullptr};
      float* Cc[2] = {pl.sage ? gWB : gWW, gWW};
      hipStream_t sw = st;
      if (big_ov && l >= 1) {
        GNN_TRY(fork_join(aux, st, aux->s));
        sw = aux->s;
        aux_used = true;
      }
      if (pl.sage && !b.xs_gathered)
        GNN_TRY(gnn::gemm_split3_indexed(1, 1, N, b.F, b.M, n, G + o, N, nullptr, 0, X + o, b.ldo, IB + o, b.K,
                                         Cc + o, b.F, b.ws_gemm_dw, b.b_gemm_dw, sw, pieces_of(b.np)));
      else
        GNN_TRY(gemm(b.np, 1, 1, N, b.F, b.M, n, G + o, N, X + o, b.ldo, Cc + o, b.F, b.ws_gemm_dw, b.b_gemm_dw, sw));
      GNN_TRY(grads_ready(2 + l, sw));  // sw follows st's norm backward (fork_join)
    } else {
      // the small weight-gradient products (rocBLAS): on the aux stream beside the input gradients
      // and the layer below (their inputs are final: the norm backward and x[sampled] / A·X)
      hipStream_t sw = st;
      rocblas_handle hw = h;
      if (ha) {
        GNN_TRY(fork_join(aux, st, aux->s));
        sw = aux->s;
        hw = ha;
        aux_used = true;
        if (head_pending) GNN_TRY(head_grads(aux->s, ha));
      }
      if (pl.sage) GNN_TRY(mm_gtx(hw, b.dhB, N, b.xs, b.ldo, gWB, b.F, N, b.F, b.M));
      GNN_TRY(mm_gtx(hw, b.dhW, N, b.feat, b.ldo, gWW, b.F, N, b.F, b.M));
      GNN_TRY(grads_ready(2 + l, sw));
    }
    if (l >= 1) {  // dY_{l-1} = A_lᵀ·dfeat (+ dxs through rmap: the x[sampled] gradient)
      LayerBufs& prev = pl.lb[l - 1];
      GNN_REQUIRE(P<const int32_t>(d, l, GNN_SL_TROWPTR) != nullptr, "gnn_train_step: layer %d has no transpose", l);
      if (pl.sage) GNN_REQUIRE(P<const int32_t>(d, l, GNN_SL_RMAP) != nullptr, "gnn_train_step: layer %d has no row map", l);
      // short-row transposes (the top layer's: 1.7 nonzeros per row on the Reddit batch) that a
      // standalone call would run as one fmaf chain per row: folded into layer l-1's tail
      // backward, which computes each dY row as it reads it (no dY write / read back, no launch)
      if (fuse_agg_enabled() && prev.D == b.F &&
          gnn::spmm_row_chain(b.K, b.M, b.nnz, b.F, b.F, b.F, b.dfeat, prev.dY)) {
        prev.dy_agg = true;
        prev.agg_rp = P<const int32_t>(d, l, GNN_SL_TROWPTR);
        prev.agg_col = P<const int32_t>(d, l, GNN_SL_TCOL);
        prev.agg_val = P<const float>(d, l, GNN_SL_TVAL);
        prev.agg_G = b.dfeat;
        prev.agg_R = pl.sage ? b.dxs : nullptr;
        prev.agg_rmap = pl.sage ? P<const int32_t>(d, l, GNN_SL_RMAP) : nullptr;
      } else if (pl.sage) {
        GNN_REQUIRE(P<const int32_t>(d, l, GNN_SL_RMAP) != nullptr, "gnn_train_step: layer %d has no row map", l);
        r.arm(1, l, b.K, b.M, b.nnz, b.F, b.F, b.F, b.F, b.dfeat, prev.dY, b.M);
        GNN_TRY(gnn_spmm_csr_f32_ex(P<const int32_t>(d, l, GNN_SL_TROWPTR), P<const int32_t>(d, l, GNN_SL_TCOL),
                                    P<const float>(d, l, GNN_SL_TVAL), b.K, b.M, b.nnz, b.dfeat, b.F, prev.dY, b.F,
                                    b.F, b.dxs, b.F, P<const int32_t>(d, l, GNN_SL_RMAP), b.ws_bwd, b.b_bwd, 0, st));
      } else {
        r.arm(1, l, b.K, b.M, b.nnz, b.F, b.F, b.F, b.F, b.dfeat, prev.dY, 0);
        GNN_TRY(gnn_spmm_csr_f32(P<const int32_t>(d, l, GNN_SL_TROWPTR), P<const int32_t>(d, l, GNN_SL_TCOL),
                                 P<const float>(d, l, GNN_SL_TVAL), b.K, b.M, b.nnz, b.dfeat, b.F, prev.dY, b.F, b.F,
                                 b.ws_bwd, b.b_bwd, 0, st));
      }
    }
  }
  if (head_pending) {  // no small weight-gradient fork above: the head's own
    GNN_TRY(fork_join(aux, st, aux->s));
    GNN_TRY(head_grads(aux->s, ha));
    aux_used = true;
  }
  if (aux_used) GNN_TRY(fork_join(aux, aux->s, st));
  return 0;
}

size_t gnn_eval_step_workspace_bytes(const int64_t* desc) {
  if (!desc) return 0;
  Arena ar{nullptr};
  Plan pl;
  if (plan_eval(desc, ar, pl)) return 0;
  return ar.off;
}

int gnn_eval_step_f32(const int64_t* d, float* logits, int64_t ldz, int32_t* counts, int mode, void* workspace,
                      size_t workspace_bytes, void* stream) {
  GNN_REQUIRE(d != nullptr, "gnn_eval_step: NULL descriptor");
  GNN_REQUIRE(d[GNN_SH_PHASE] == 0, "gnn_eval_step: phase %lld (must be 0)", (long long)d[GNN_SH_PHASE]);
  GNN_REQUIRE(mode == 0 || mode == 1, "gnn_eval_step: mode %d", mode);
  const float* labels = HP<const float>(d, GNN_SH_LABELS);
  float* loss = HP<float>(d, GNN_SH_LOSS);
  GNN_REQUIRE((labels != nullptr) == (loss != nullptr) && (!labels || counts),
              "gnn_eval_step: labels, loss and counts come together (all NULL: predict)");
  GNN_REQUIRE(labels || logits, "gnn_eval_step: nothing to produce (no labels, no logits)");
  Arena ar{(char*)workspace};
  Run r;
  Plan& pl = r.pl;
  {
    Arena dry{nullptr};
    Plan tmp;
    GNN_TRY(plan_eval(d, dry, tmp));
    GNN_TRY(check_workspace(workspace, workspace_bytes, dry.off));
    GNN_REQUIRE((!logits || ldz >= tmp.C) && (!labels || d[GNN_SH_LDL] >= tmp.C),
                "gnn_eval_step: logits / labels row stride below %lld classes", (long long)tmp.C);
  }
  GNN_TRY(plan_eval(d, ar, pl));
  GNN_TRY(r.open(d, (hipStream_t)stream));
  GNN_TRY(forward(r));  // training = 0, no timing records, phase 0
  const LayerBufs& top = pl.lb[pl.nl - 1];
  return gnn_head_eval_loss_f32(top.Y, top.D, pl.Mh, pl.Dh, HP<const float>(d, GNN_SH_HEAD_W),
                                HP<const float>(d, GNN_SH_HEAD_B), pl.C, labels, d[GNN_SH_LDL], logits, ldz,
                                pl.rowloss, pl.rowmask, loss, counts, mode, pl.loss_kind, stream);
}

}  // extern "C"
