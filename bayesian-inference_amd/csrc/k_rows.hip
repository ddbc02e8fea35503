// The plumbing the summaries of a stored chain share (rows_dev.h): the gather of a view of rows in blocks,
// the pooled moments, the workspace budget and the key-only radix sort of rows.  The radix select is k_select.hip, the
// histogram sweep k_marginal.hip; the summaries' own kernels are not here.
//
// The sort: the key-only LSD radix sort of rows of doubles that the exact ranks (k_diag.hip) and the highest-density intervals
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
// of rows or on the run.  The pass count is fixed, whatever the data.  The kernels are compiled once, here.
#include "rows_dev.h"
#include "wg_dev.h"

namespace gpemu {

// ---- rows in blocks ------------------------------------------------------------------------------------------------
int rows_check(const RowsView &v) {
  GP_ARG(v.n_blocks > 0 && v.block_rows > 0, "n_blocks and block_rows must be positive");
  GP_ARG(v.d >= 1, "d must be positive");
  GP_ARG(v.n_blocks == 1 || v.block_stride / v.d >= v.block_rows, "the stride between blocks must hold a block");
  return GPEMU_OK;
}

int rows_view(const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows, int d, RowsView *v) {
  GP_ARG(d >= 1 && d <= ROWS_MAX_D, "d must be in [1, 16]");
  *v = RowsView{dX, n_blocks, block_rows, block_stride_rows * d, d};
  GP_TRY(rows_check(*v));
  GP_ARG(n_blocks <= ((1ll << 31) - 1) / block_rows, "S = n_blocks * block_rows must be below 2^31");
  return GPEMU_OK;
}

// dst[n][d] = logical rows [r0, r0 + n) of v
__global__ __launch_bounds__(256) void gather_rows_kernel(RowsView v, int64_t r0, int64_t n, double *__restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * v.d) return;
  dst[i] = v.row(r0 + i / v.d)[i % v.d];
}

int gather_rows(const RowsView &v, int64_t r0, int64_t n, double *dst, hipStream_t st) {
  const int64_t per = std::max<int64_t>(1, (256ll * 0x7fffffff) / v.d);   // rows of one launch: the grid is 32 bits wide
  for (int64_t a = 0; a < n; a += per) {
    const int64_t m = std::min(per, n - a);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((m * v.d + 255) / 256)), dim3(256), 0, st, v, r0 + a, m,
                       dst + a * v.d);
    GP_HIP(hipGetLastError());
  }
  return GPEMU_OK;
}

// ---- pooled mean and variance per parameter, two passes, tree A (wg_dev.h) ---------------------------------------
// (MOM_ROWS rows of the flattened chain [R][d] per workgroup)

// part[b][dd] = sum over the rows of block b of x (mean == null) or of (x - mean[dd])^2
__global__ __launch_bounds__(256) void moments_partial_kernel(const double *__restrict__ x, int64_t R, int d,
                                                              const double *__restrict__ mean, double *__restrict__ part) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * MOM_ROWS, r1 = (r0 + MOM_ROWS < R) ? r0 + MOM_ROWS : R;
  for (int dd = 0; dd < d; ++dd) {
    const double mu = mean ? mean[dd] : 0.0;
    double s = 0.0;
    for (int64_t r = r0 + t; r < r1; r += 256) {
      const double v = x[r * d + dd] - mu;
      s += mean ? v * v : v;
    }
    s = wg_sum_a<256>(s, red);
    if (t == 0) part[(int64_t)blockIdx.x * d + dd] = s;
  }
}

// out[e] = (sum over the blocks of part[b][e]) / R; grid = nent workgroups
__global__ __launch_bounds__(256) void moments_final_kernel(const double *__restrict__ part, int64_t nb, int nent, int64_t R,
                                                            double *__restrict__ out) {
  __shared__ double red[256];
  const int t = threadIdx.x, e = blockIdx.x;
  double s = 0.0;
  for (int64_t b = t; b < nb; b += 256) s += part[b * nent + e];
  s = wg_sum_a<256>(s, red);
  if (t == 0) out[e] = s / (double)R;
}

void launch_moments_final(const double *dpart, int64_t nb, int nent, int64_t R, double *dout, hipStream_t st) {
  hipLaunchKernelGGL(moments_final_kernel, dim3((unsigned)nent), dim3(256), 0, st, dpart, nb, nent, R, dout);
}

int launch_moments(const double *dx, int64_t R, int d, double *dpart, double *dmom, hipStream_t st) {
  const int64_t nb = (R + MOM_ROWS - 1) / MOM_ROWS;
  hipLaunchKernelGGL(moments_partial_kernel, dim3((unsigned)nb), dim3(256), 0, st, dx, R, d, (const double *)nullptr, dpart);
  launch_moments_final(dpart, nb, d, R, dmom, st);
  hipLaunchKernelGGL(moments_partial_kernel, dim3((unsigned)nb), dim3(256), 0, st, dx, R, d, (const double *)dmom, dpart);
  launch_moments_final(dpart, nb, d, R, dmom + d, st);
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

int moments_to_host(const double *dx, int64_t R, int d, double *mean, double *var, hipStream_t st) {
  DevScope sc(st);
  double *dpart = nullptr, *dmom = nullptr;
  GP_TRY(sc.alloc(&dpart, (R + MOM_ROWS - 1) / MOM_ROWS * d));
  GP_TRY(sc.alloc(&dmom, 2 * d));
  GP_TRY(launch_moments(dx, R, d, dpart, dmom, st));
  GP_TRY(sc.download(mean, dmom, d));
  GP_TRY(sc.download(var, dmom + d, d));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

// ---- workspace budget ----------------------------------------------------------------------------------------------
int workspace_budget(int64_t workspace_bytes, int64_t *budget) {
  *budget = workspace_bytes;
  if (workspace_bytes == 0) {
    size_t fb = 0, tb = 0;
    GP_HIP(hipMemGetInfo(&fb, &tb));
    *budget = (int64_t)(fb / 2);
  }
  return GPEMU_OK;
}

const char *workspace_budget_name(int64_t workspace_bytes) {
  return workspace_bytes ? "allowed by workspace_bytes" : "available (half of the free device memory)";
}

// ---- the sort ---------------------------------------------------------------------------------------------------------
constexpr int RK_ROUNDS = RK_TILE / 256;

// keys[rl][i] = key of element i of row row0 + rl; nan[rl] = 1 if the row holds a NaN.  Workgroup (rl, 256 elements)
__global__ __launch_bounds__(256) void rk_key_kernel(const double *V, int64_t row_stride, int64_t elem_stride, int64_t S,
                                                     int64_t row0, int64_t nblk, u64 *__restrict__ keys,
                                                     int *__restrict__ nan) {
  const int64_t rl = blockIdx.x / nblk, i = (blockIdx.x % nblk) * 256 + threadIdx.x;
  if (i >= S) return;
  const double v = V[(row0 + rl) * row_stride + i * elem_stride];
  if (v != v) nan[rl] = 1;
  keys[rl * S + i] = rk_key(v);
}

// hist[(rl 256 + digit) ntiles + tile] = number of keys of the tile with that digit
__global__ __launch_bounds__(256) void rk_hist_kernel(const u64 *__restrict__ keys, int64_t S, int64_t ntiles, int shift,
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
__global__ __launch_bounds__(256) void rk_scan_kernel(unsigned *__restrict__ hist, int64_t ntiles) {
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
__global__ __launch_bounds__(256) void rk_scatter_kernel(const u64 *__restrict__ src, u64 *__restrict__ dst, int64_t S,
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

int64_t sort_rows_cap(int64_t R, int64_t S, int64_t budget, int64_t per_row, int64_t grid_per_row) {
  int64_t cap = std::min<int64_t>(R, budget / per_row);
  cap = std::min<int64_t>(cap, (int64_t)0x7fffffff / ((S + 255) / 256));   // the grids are (rows, blocks) flattened
  return std::min<int64_t>(cap, (int64_t)0x7fffffff / grid_per_row);
}

int SortScratch::alloc(DevScope &sc, int64_t rows_cap, int64_t S) {
  GP_TRY(sc.alloc(&ka, rows_cap * S));
  GP_TRY(sc.alloc(&kb, rows_cap * S));
  GP_TRY(sc.alloc(&hist, rows_cap * RK_BINS * ((S + RK_TILE - 1) / RK_TILE)));
  GP_TRY(sc.alloc(&nan, rows_cap));
  return GPEMU_OK;
}

// the keys into s.ka, then the RK_PASSES passes between s.ka and s.kb: an even number, so the sorted keys end in s.ka
int sort_rows(const double *dV, int64_t row_stride, int64_t elem_stride, int64_t S, int64_t row0, int64_t rows,
              const SortScratch &s, void (*on_pass)(), hipStream_t st) {
  const int64_t ntiles = (S + RK_TILE - 1) / RK_TILE, nblk = (S + 255) / 256;
  GP_HIP(hipMemsetAsync(s.nan, 0, sizeof(int) * (size_t)rows, st));
  hipLaunchKernelGGL(rk_key_kernel, dim3((unsigned)(rows * nblk)), dim3(256), 0, st, dV, row_stride, elem_stride, S, row0,
                     nblk, s.ka, s.nan);
  GP_HIP(hipGetLastError());
  u64 *src = s.ka, *dst = s.kb;
  for (int pass = 0; pass < RK_PASSES; ++pass) {
    on_pass();
    hipLaunchKernelGGL(rk_hist_kernel, dim3((unsigned)(rows * ntiles)), dim3(256), 0, st, src, S, ntiles, 8 * pass, s.hist);
    hipLaunchKernelGGL(rk_scan_kernel, dim3((unsigned)rows), dim3(256), 0, st, s.hist, ntiles);
    hipLaunchKernelGGL(rk_scatter_kernel, dim3((unsigned)(rows * ntiles)), dim3(256), 0, st, src, dst, S, ntiles, 8 * pass,
                       s.hist);
    GP_HIP(hipGetLastError());
    std::swap(src, dst);
  }
  return GPEMU_OK;
}

}  // namespace gpemu
