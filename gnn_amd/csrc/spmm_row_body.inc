// spmm_row_body.inc — the body of spmm_row_kernel (fp32 X) and spmm_row16_kernel (16-bit X),
// included by spmm.hip inside each kernel (see spmm_unit_body.inc). The including kernel provides
// VW, NJ, U, WPR, RES, XK and the parameters.
  using V = typename Vec<VW>::T;
  using XL = XLoad<XK, VW>;
  using XV = typename XL::T;
  constexpr int COVER = 64 * VW * NJ;
  __shared__ V part[WPR > 1 ? WPR - 1 : 1][NJ][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int r = (int)(blockIdx.x / (unsigned)slices);
  const int s = (int)(blockIdx.x - (unsigned)r * (unsigned)slices);
  if (r >= M) return;
  const int c0 = s * COVER + lane * VW;
  int q = -1;
  if constexpr (RES) q = rmap[r];  // issued early: its latency overlaps the walk
  const int rb = rowptr[r];
  const int re = rowptr[r + 1];
  const int per = (re - rb + WPR - 1) / WPR;
  const int b = rb + w * per;
  const int e = min(re, b + per);
  V acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = vzero<VW>();
  for (int base = b; base < e; base += 64) {
    const int n = min(64, e - base);
    int mc = 0;
    float mv = 0.0f;
    if (lane < n) {
      mc = col[base + lane];
      mv = val[base + lane];
    }
    for (int k = 0; k < n; k += U) {
      XV xs[U][NJ];
      float vs[U];
#pragma unroll
      for (int t = 0; t < U; ++t) {
        const int idx = k + t;  // wave-uniform
        if (idx >= n) {        // past the chunk: no load, the FMA adds 0 * 0
          vs[t] = 0.0f;
#pragma unroll
          for (int j = 0; j < NJ; ++j) xs[t][j] = XV(0);
          continue;
        }
        const int c = readlane_i(mc, idx);  // scalar row address
        vs[t] = readlane_f(mv, idx);
        const typename XL::E* xr = X + (int64_t)c * ldx;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int cc = min(c0 + j * 64 * VW, F - VW);  // past F: the row's last vector (unstored)
          xs[t][j] = *reinterpret_cast<const XV*>(xr + cc);
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // all U * NJ row loads ahead of the FMAs
#pragma unroll
      for (int t = 0; t < U; ++t) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = vfma(vs[t], XL::widen(xs[t][j]), acc[j]);
      }
    }
  }
  if constexpr (WPR > 1) {
    if (w > 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) part[w - 1][j][lane] = acc[j];
    }
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int p = 0; p < WPR - 1; ++p) {  // wave order: deterministic
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] += part[p][j][lane];
    }
  }
  float* dst = Y + (int64_t)r * ldy;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int cc = c0 + j * 64 * VW;
    if (cc < F) {
      V a = acc[j];
      if constexpr (RES) {
        if (q >= 0) a += *reinterpret_cast<const V*>(R + (int64_t)q * ldr + cc);
      }
      *reinterpret_cast<V*>(dst + cc) = a;
    }
  }
