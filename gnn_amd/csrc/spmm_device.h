// spmm_device.h — device helpers shared by spmm.hip, operand.hip and gather.hip: the float vector
// types and their FMA / shuffle forms, the readlane wrappers and the wave-wide search. Private to
// csrc/; each translation unit gets its own (internal-linkage, always inlined) copies.
#pragma once

#include <hip/hip_runtime.h>

namespace {

// ---------------------------------------------------------------------------------
// Vector types: clang ext vectors give global_load_dwordx2/x4 and per-lane packed FMA.
// ---------------------------------------------------------------------------------
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
template <int VW> struct Vec;
template <> struct Vec<1> { using T = float; };
template <> struct Vec<2> { using T = f2; };
template <> struct Vec<4> { using T = f4; };

template <int VW>
__device__ __forceinline__ typename Vec<VW>::T vzero() { return typename Vec<VW>::T(0.0f); }

// acc + v * x with one rounding per element (matches a C fmaf chain bit for bit).
__device__ __forceinline__ float vfma(float v, float x, float acc) { return __builtin_fmaf(v, x, acc); }
__device__ __forceinline__ f2 vfma(float v, f2 x, f2 acc) {
  return f2{__builtin_fmaf(v, x.x, acc.x), __builtin_fmaf(v, x.y, acc.y)};
}
__device__ __forceinline__ f4 vfma(float v, f4 x, f4 acc) {
  return f4{__builtin_fmaf(v, x.x, acc.x), __builtin_fmaf(v, x.y, acc.y),
            __builtin_fmaf(v, x.z, acc.z), __builtin_fmaf(v, x.w, acc.w)};
}

__device__ __forceinline__ float shfl_xor_v(float x, int m) { return __shfl_xor(x, m); }
__device__ __forceinline__ f2 shfl_xor_v(f2 x, int m) { return f2{__shfl_xor(x.x, m), __shfl_xor(x.y, m)}; }
__device__ __forceinline__ f4 shfl_xor_v(f4 x, int m) {
  return f4{__shfl_xor(x.x, m), __shfl_xor(x.y, m), __shfl_xor(x.z, m), __shfl_xor(x.w, m)};
}

__device__ __forceinline__ int readlane_i(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ float readlane_f(float x, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}

// Smallest r in [lo, hi) with pred(r) true (pred monotone false..true), hi if none.
// 64 probes per round: ceil(log64(hi-lo)) dependent rounds (3 for 250k rows).
template <class Pred>
__device__ __forceinline__ int wave_first_true(int lo, int hi, int lane, Pred pred) {
  while (lo < hi) {
    const int n = hi - lo;
    const int step = (n + 63) >> 6;
    const int r = lo + lane * step;
    const bool p = (r < hi) && pred(r);
    const unsigned long long b = __ballot(p);
    if (b == 0ull) {
      lo = lo + ((n - 1) / step) * step + 1;
    } else {
      const int f = __builtin_ctzll(b);
      hi = lo + f * step;
      lo = (f == 0) ? hi : lo + (f - 1) * step + 1;
    }
  }
  return lo;
}

}  // namespace
