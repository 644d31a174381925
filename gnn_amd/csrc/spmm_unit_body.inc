// spmm_unit_body.inc — the body of spmm_unit_kernel (fp32 X) and spmm_unit16_kernel (16-bit X),
// included by spmm.hip inside each kernel: one text, so the two walk, sum and store alike, while the
// fp32 kernel keeps its name and its code. The including kernel provides VW, G, NJ, U, RES, XK and
// the parameters named below (spmm.hip documents them).
  using V = typename Vec<VW>::T;
  using XL = XLoad<XK, VW>;
  using XV = typename XL::T;
  constexpr int P = 64 / G;            // nonzeros taken side by side per step
  constexpr int COVER = VW * G * NJ;   // columns covered by one column tile
  const int lane = threadIdx.x & 63;
  int ub, tile;
  if (!wm.locate(blockIdx.x, ub, tile)) return;
  const int u = ub * 4 + (threadIdx.x >> 6);  // wave-uniform; no block barriers below
  const int sub = lane / G;
  const int c0 = tile * COVER + (lane % G) * VW;
  if (u >= nunits) {  // row unit: the empty rows among ROW_UNIT consecutive rows
    const int r0 = (u - nunits) * ROW_UNIT;
    if (r0 >= M) return;
    const int rl = r0 + lane;
    unsigned long long em = __ballot(rl < M && rowptr[rl] == rowptr[rl + 1]);
    while (em) {
      const int r = r0 + __builtin_ctzll(em);
      em &= em - 1;
      const float* res = nullptr;
      if constexpr (RES) {
        const int q = rmap[r];
        if (q >= 0) res = R + (int64_t)q * ldr;
      }
      float* dst = Y + (int64_t)r * ldy;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cc = c0 + j * G * VW;
        if ((j % P) == sub && cc < F) {
          V a = vzero<VW>();
          if constexpr (RES) {
            if (res) a = *reinterpret_cast<const V*>(res + cc);
          }
          *reinterpret_cast<V*>(dst + cc) = a;
        }
      }
    }
    return;
  }

  const int ustart = u * S;  // host guarantees nunits * S fits in int
  const int uend = min(ustart + S, nnz);

  // Row ownership: a row of at most S nonzeros belongs wholly to the unit holding its first
  // nonzero (it may run past uend, by < S); only longer rows are cut at unit boundaries.
  // rlo = the row containing position ustart (or the first row starting at/after it).
  const int rlo = wave_first_true(0, M, lane, [&](int r) {
    return rowptr[r + 1] > ustart || rowptr[r] >= ustart;
  });
  // (rows starting at or after uend belong to later units; trailing empty rows start at nnz)
  const int rhi = wave_first_true(rlo, M, lane, [&](int r) { return rowptr[r] >= uend; });

  for (int r = rlo; r < rhi; ++r) {
    const int rb = rowptr[r];
    const int re = rowptr[r + 1];
    if (rb == re) {  // empty: a row unit stores it; skip the whole run of empty rows at rb
      r = wave_first_true(r + 1, rhi, lane, [&](int q) { return rowptr[q + 1] > rb; }) - 1;
      continue;
    }
    const bool cut = re - rb > S;  // wave-uniform
    if (rb < ustart && !cut) continue;  // short row owned by an earlier unit
    const int b = max(rb, ustart);
    const int e = cut ? min(re, uend) : re;
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
      const int last_c = __shfl(mc, n - 1);
      for (int k = 0; k < n; k += P * U) {
        XV xs[U][NJ];
        float vs[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
          const int idx = k + t * P + sub;
          int c;
          float v;
          // idx may run past the chunk (and past lane 63, where lane selects wrap):
          // such padded slots get v = 0 and re-read a row already in flight.
          if constexpr (P == 1) {
            c = readlane_i(mc, idx & 63);  // idx is wave-uniform: scalar row address
            v = readlane_f(mv, idx & 63);
          } else {
            c = __shfl(mc, idx & 63);
            v = __shfl(mv, idx & 63);
          }
          if (idx >= n) {
            c = last_c;
            v = 0.0f;
          }
          vs[t] = v;
          const typename XL::E* xr = X + (int64_t)c * ldx;
          // a slot past the row end for every lane group (the row's last, partly empty round:
          // 6-7 % of the slots on the Reddit layers) issues no load; its FMA adds 0 * 0, as the
          // loaded-and-masked slot added 0 * x: bit-identical (A/B: layer-0 forward -1 %)
          if (k + t * P >= n) {  // wave-uniform
#pragma unroll
            for (int j = 0; j < NJ; ++j) xs[t][j] = XV(0);
            continue;
          }
          // Columns past F load the row's last vector instead (same cache lines, no
          // branch, no extra HBM bytes); those accumulator slots are never stored.
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int cc = min(c0 + j * G * VW, F - VW);
            xs[t][j] = *reinterpret_cast<const XV*>(xr + cc);
          }
        }
        // keep all U * NJ row loads ahead of the FMAs (the scheduler otherwise interleaves
        // them to raise occupancy, leaving fewer loads in flight per wave)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < U; ++t) {
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[j] = vfma(vs[t], XL::widen(xs[t][j]), acc[j]);
        }
      }
    }

    if constexpr (P > 1) {
#pragma unroll
      for (int m = G; m < 64; m <<= 1) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] += shfl_xor_v(acc[j], m);
      }
    }

    float* dst;
    const float* res = nullptr;  // residual row added to a complete output row
    if (!cut) {
      dst = Y + (int64_t)r * ldy;
      if constexpr (RES) {
        const int q = rmap[r];
        if (q >= 0) res = R + (int64_t)q * ldr;
      }
    } else {
      dst = slab + ((int64_t)u * 2 + (rb < ustart ? 0 : 1)) * ldslab;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int cc = c0 + j * G * VW;
      if ((j % P) == sub && cc < F) {
        V a = acc[j];
        if constexpr (RES) {
          if (res) a += *reinterpret_cast<const V*>(res + cc);
        }
        *reinterpret_cast<V*>(dst + cc) = a;
      }
    }
  }
