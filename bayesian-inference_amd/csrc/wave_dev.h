// The wave-level primitives every kernel family shares (one wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>

namespace gpemu {

// the sum of `v` over the wave's 64 lanes, in every lane: the xor butterfly 32, 16, ... 1 (one fixed tree: the bits
// depend on the values alone)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the same butterfly on 64-bit integers: the sum of `v` over the wave's 64 lanes, in every lane
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the maximum of `v` over the wave's 64 lanes, in every lane: the same butterfly with fmax (NaN is passed over)
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// value of lane `l` (compile-time / wave-uniform index) as a scalar: v_readlane, no LDS round trip
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// the wave's LDS writes so far are visible to its other lanes' reads that follow
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace gpemu
