// The two workgroup reductions of one value per thread.  Each is one fixed summation tree: the bits of a
// result depend on the values and on the tree alone, never on the grid, the batch or the run.
//
// Tree A, "LDS tree" (wg_tree_a; wg_sum_a, wg_min_a, wg_max_a).  Every thread stores its value at red[t].  After a
// barrier, for off = THREADS/2, ..., 1, thread t < off does red[t] = op(red[t], red[t + off]), with a barrier after each
// level.  The result is red[0].
//
// Tree B, "wave tree" (wg_tree_b; wg_sum_b, wg_max_b).  The xor butterfly 32 ... 1 runs within each wave (wave_sum,
// wave_max).  Lane 0 of wave w then stores to ws[w].  After a barrier, the waves are combined left to right:
// ((ws[0] op ws[1]) op ws[2]) op ...
//
// A and B give different bits for doubles: A combines across waves first and B combines last.  A double sum must
// therefore name its tree.  A new kernel picks B (two barriers and WAVES doubles of LDS) unless it must match an
// existing A result.  Integer sums, fmin and fmax are order-independent and may use either.
//
// Both return the result in every thread and end with a barrier, so the caller's scratch (red[THREADS], ws[WAVES]) can
// be reused at once.  Every thread of the workgroup must call; the workgroup has THREADS = 64 WAVES threads.
#pragma once
#include "wave_dev.h"

namespace gpemu {

// the operations: op(a, b), and for tree B the same operation over a wave (wave_dev.h)
struct OpSum {
  template <class T> __device__ T operator()(T a, T b) const { return a + b; }
  __device__ double wave(double v) const { return wave_sum(v); }
};
struct OpMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct OpMax {
  __device__ double operator()(double a, double b) const { return fmax(a, b); }
  __device__ double wave(double v) const { return wave_max(v); }
};

// ---- tree A --------------------------------------------------------------------------------------------------------
template <int THREADS, class T, class Op>
__device__ __forceinline__ T wg_tree_a(T v, T *red, Op op) {
  static_assert(THREADS >= 2 && (THREADS & (THREADS - 1)) == 0, "a power of two");
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int off = THREADS / 2; off > 0; off >>= 1) {
    if (t < off) red[t] = op(red[t], red[t + off]);
    __syncthreads();
  }
  const T out = red[0];
  __syncthreads();
  return out;
}
template <int THREADS, class T>
__device__ __forceinline__ T wg_sum_a(T v, T *red) { return wg_tree_a<THREADS>(v, red, OpSum{}); }
template <int THREADS>
__device__ __forceinline__ double wg_min_a(double v, double *red) { return wg_tree_a<THREADS>(v, red, OpMin{}); }
template <int THREADS>
__device__ __forceinline__ double wg_max_a(double v, double *red) { return wg_tree_a<THREADS>(v, red, OpMax{}); }

// ---- tree B --------------------------------------------------------------------------------------------------------
template <int WAVES, class Op>
__device__ __forceinline__ double wg_tree_b(double v, double *ws, Op op) {
  v = op.wave(v);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  double out = ws[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) out = op(out, ws[w]);
  __syncthreads();
  return out;
}
template <int WAVES>
__device__ __forceinline__ double wg_sum_b(double v, double *ws) { return wg_tree_b<WAVES>(v, ws, OpSum{}); }
template <int WAVES>
__device__ __forceinline__ double wg_max_b(double v, double *ws) { return wg_tree_b<WAVES>(v, ws, OpMax{}); }

}  // namespace gpemu
