// The key-only LSD radix sort of rows of doubles that the exact ranks (k_diag.hip) and the highest-density intervals
// (k_marginal.hip) share: order-preserving 64-bit keys (sel_key; -0 canonicalised to +0 first), RK_PASSES = 8 stable
// passes of 8 bits, least significant byte first.  Per pass
//   rk_hist_kernel     workgroup (row, tile) counts the digits of its RK_TILE keys into an LDS histogram (LDS integer
//                      atomics) and stores it at hist[row][digit][tile];
//   rk_scan_kernel     one workgroup per row: exclusive scan of the row's hist over (digit, tile), digit major -- the
//                      first output position of every (digit, tile);
//   rk_scatter_kernel  workgroup (row, tile): wave w owns keys [512 w, 512 w + 512) of the tile, in 8 rounds of 64
//                      consecutive keys.  The waves count their digits (LDS integer atomics), one thread per digit turns
//                      the counts into the waves' first positions, and every wave places its rounds in order: the lanes
//                      with one digit find each other with 8 ballots (64-bit masks), a lane's place is the group's
//                      position + the number of lower lanes in the group, and the group's lowest lane advances the
//                      wave's own LDS counter.  Equal digits keep their order: the pass is stable.
// The sorted key array of a row is unique and every counter is an integer: it does not depend on the grid, on the batch
// of rows or on the run.  The pass count is fixed, whatever the data.  The kernels are static: each file that includes
// this header launches its own copies.
#pragma once
#include <algorithm>

#include "internal.h"
#include "sampler_internal.h"

namespace gpemu {

constexpr int RK_PASSES = 8;       // 8 bits each
constexpr int RK_BINS = 256;
constexpr int RK_TILE = 2048;      // keys per workgroup: 4 waves x 8 rounds x 64 lanes
constexpr int RK_ROUNDS = RK_TILE / 256;

static __device__ __forceinline__ u64 rk_key(double v) {
  if (v == 0.0) v = 0.0;   // -0 and +0 are tied
  return sel_key(v);
}

// keys[rl][i] = key of element i of row row0 + rl; nan[rl] = 1 if the row holds a NaN.  Workgroup (rl, 256 elements)
static __global__ __launch_bounds__(256) void rk_key_kernel(const double *V, int64_t row_stride, int64_t elem_stride, int64_t S,
                                                     int64_t row0, int64_t nblk, u64 *__restrict__ keys,
                                                     int *__restrict__ nan) {
  const int64_t rl = blockIdx.x / nblk, i = (blockIdx.x % nblk) * 256 + threadIdx.x;
  if (i >= S) return;
  const double v = V[(row0 + rl) * row_stride + i * elem_stride];
  if (v != v) nan[rl] = 1;
  keys[rl * S + i] = rk_key(v);
}

// hist[(rl 256 + digit) ntiles + tile] = number of keys of the tile with that digit
static __global__ __launch_bounds__(256) void rk_hist_kernel(const u64 *__restrict__ keys, int64_t S, int64_t ntiles, int shift,
                                                      unsigned *__restrict__ hist) {
  __shared__ unsigned h[RK_BINS];
  const int tid = threadIdx.x;
  const int64_t rl = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
  h[tid] = 0;
  __syncthreads();
  const u64 *row = keys + rl * S;
#pragma unroll
  for (int r = 0; r < RK_ROUNDS; ++r) {
    const int64_t i = tile * RK_TILE + r * 256 + tid;
    if (i < S) atomicAdd(&h[(unsigned)(row[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(rl * RK_BINS + tid) * ntiles + tile] = h[tid];
}

// in place: hist[rl][j] -> the sum of hist[rl][0 .. j), j over (digit, tile) digit major; one workgroup per row, thread
// t owns digit t, the entries [t ntiles, (t + 1) ntiles)
static __global__ __launch_bounds__(256) void rk_scan_kernel(unsigned *__restrict__ hist, int64_t ntiles) {
  __shared__ unsigned tot[256];
  const int tid = threadIdx.x;
  const int64_t L = RK_BINS * ntiles;      // = 256 ntiles: every thread owns ntiles entries, one digit
  unsigned *h = hist + (int64_t)blockIdx.x * L + (int64_t)tid * ntiles;
  unsigned s = 0;
  for (int64_t j = 0; j < ntiles; ++j) s += h[j];
  tot[tid] = s;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {   // inclusive scan of the 256 digit totals
    const unsigned add = tid >= off ? tot[tid - off] : 0u;
    __syncthreads();
    tot[tid] += add;
    __syncthreads();
  }
  unsigned run = tot[tid] - s;
  for (int64_t j = 0; j < ntiles; ++j) {
    const unsigned c = h[j];
    h[j] = run;
    run += c;
  }
}

// the stable scatter of one pass: dst[rl][position] = key (the file's header)
static __global__ __launch_bounds__(256) void rk_scatter_kernel(const u64 *__restrict__ src, u64 *__restrict__ dst, int64_t S,
                                                         int64_t ntiles, int shift, const unsigned *__restrict__ offs) {
  __shared__ unsigned wh[4 * RK_BINS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t rl = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
#pragma unroll
  for (int j = 0; j < 4; ++j) wh[j * RK_BINS + tid] = 0;
  __syncthreads();
  const u64 *row = src + rl * S;
  u64 *out = dst + rl * S;
  const int64_t base = tile * RK_TILE + wave * (RK_ROUNDS * 64) + lane;
  u64 key[RK_ROUNDS];
#pragma unroll
  for (int r = 0; r < RK_ROUNDS; ++r) {
    const int64_t i = base + r * 64;
    key[r] = 0;
    if (i < S) {
      key[r] = row[i];
      atomicAdd(&wh[wave * RK_BINS + ((unsigned)(key[r] >> shift) & 255u)], 1u);
    }
  }
  __syncthreads();
  {   // thread = digit: the counts of the waves become their first positions
    unsigned b = offs[(rl * RK_BINS + tid) * ntiles + tile];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned c = wh[j * RK_BINS + tid];
      wh[j * RK_BINS + tid] = b;
      b += c;
    }
  }
  __syncthreads();
  volatile unsigned *mine = wh + wave * RK_BINS;   // this wave's counters: read and advanced in program order
  const u64 below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < RK_ROUNDS; ++r) {
    const bool valid = base + r * 64 < S;
    const unsigned digit = (unsigned)(key[r] >> shift) & 255u;
    u64 same = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (digit >> bit) & 1u;
      const u64 b = __ballot(one);
      same &= one ? b : ~b;
    }
    if (valid) {
      const unsigned before = (unsigned)__popcll(same & below);
      const unsigned pos = mine[digit] + before;
      if ((int64_t)pos < S) out[pos] = key[r];
      if (before == 0) mine[digit] = pos + (unsigned)__popcll(same);
    }
  }
}

// bytes of the sort's buffers for one row of S elements: two key arrays, the (digit, tile) histogram, the NaN flag
static inline int64_t rank_row_bytes(int64_t S) { return 16 * S + 4 * RK_BINS * ((S + RK_TILE - 1) / RK_TILE) + 4; }

// keys of `rows` rows from row0 on into ka, then the RK_PASSES passes between ka and kb: the sorted keys end in ka (an
// even number of passes).  nan[rl] = 1 for a row that holds a NaN.  on_pass() is called once per pass (path counters).
static int sort_rows(const double *dV, int64_t row_stride, int64_t elem_stride, int64_t S, int64_t row0, int64_t rows,
                     u64 *ka, u64 *kb, unsigned *hist, int *nan, void (*on_pass)(), hipStream_t st) {
  const int64_t ntiles = (S + RK_TILE - 1) / RK_TILE, nblk = (S + 255) / 256;
  GP_HIP(hipMemsetAsync(nan, 0, sizeof(int) * (size_t)rows, st));
  hipLaunchKernelGGL(rk_key_kernel, dim3((unsigned)(rows * nblk)), dim3(256), 0, st, dV, row_stride, elem_stride, S, row0,
                     nblk, ka, nan);
  GP_HIP(hipGetLastError());
  u64 *src = ka, *dst = kb;
  for (int pass = 0; pass < RK_PASSES; ++pass) {
    on_pass();
    hipLaunchKernelGGL(rk_hist_kernel, dim3((unsigned)(rows * ntiles)), dim3(256), 0, st, src, S, ntiles, 8 * pass, hist);
    hipLaunchKernelGGL(rk_scan_kernel, dim3((unsigned)rows), dim3(256), 0, st, hist, ntiles);
    hipLaunchKernelGGL(rk_scatter_kernel, dim3((unsigned)(rows * ntiles)), dim3(256), 0, st, src, dst, S, ntiles, 8 * pass,
                       hist);
    GP_HIP(hipGetLastError());
    std::swap(src, dst);
  }
  return GPEMU_OK;
}

}  // namespace gpemu
