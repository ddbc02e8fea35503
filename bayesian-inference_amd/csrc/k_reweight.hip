// Importance reweighting of a stored chain and its weighted summaries (gpemu_logprior*, gpemu_logmeanexp_dev,
// gpemu_weights_fixed_dev, gpemu_weighted_select*, gpemu_weighted_hist*): the posterior under another prior
// or under other data, from the chain that exists.
//
//   logprior_kernel    one lane per sample of the block layout; the scenario tables (kind, a, b)[R][d] sit in LDS;
//                      L[r][s] = sum_i f_ri(x_si), added in index order, one rounding per addition.
//   lse_max_kernel / lse_sum_kernel with their finish kernels: the log-sum-exp of every row over chunks of RW_SUM = 4096
//                      fixed by the index (a lane adds its 16 elements in index order, then tree B of wg_dev.h, the
//                      chunks in order), and on request L - logsumexp(L).
//   quantise_kernel    q = (u64) rint(exp(lw) 2^52); Q[r] = the integer sum of the row (tree A on integers, then one
//                      64-bit global integer atomic per workgroup).
//   wsel_hist_kernel / wsel_scan_kernel: the radix select of k_postpred.hip (order-preserving key, eight passes of 8
//                      bits, most significant first, slots shared by targets whose prefixes agree) with histograms of
//                      WEIGHT SUMS: 64-bit LDS integer atomics, non-zero bins flushed with 64-bit global integer atomics;
//                      the scan walks the cumulative weight to the target and keeps the remaining target within the bin.
//                      A "row" of the state is a (weight row, value row) pair.  A sample's weight is loaded only when its
//                      key matches a live prefix; a sample of weight 0 adds nothing.
//   whist_kernel       the sweep of k_marginal.hip's histogram with 64-bit bins in LDS that take q instead of 1: 18432
//                      bins per sweep (144 KiB), so a pair whose nb2^2 bins do not fit is swept in bands of its first
//                      index.  grid.y = the weight row.
// Every weight is an integer and every sum of a row's weights is below 2^53: no result depends on the order of the
// atomics, on the grid, on the batches or on the run.  No floating-point atomics.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "internal.h"
#include "rows_dev.h"
#include "sampler_internal.h"
#include "wg_dev.h"

namespace gpemu {

constexpr int RW_MAX_D = 16;
constexpr int RW_MAX_R = 64;           // scenarios per logprior call
constexpr int64_t RW_SUM = 4096;       // samples per partial sum
constexpr int WS_PASSES = 8;           // 8 bits each
constexpr int WS_BINS = 256;
constexpr int WS_MAXT = 16;            // targets (and slots) per group
constexpr int WS_ROWS = 512;           // (weight row, value row) pairs per batch, at most
constexpr int64_t WS_SLICE = 4096;     // least elements per workgroup
constexpr int64_t WS_MAX_WG = 8192;    // workgroups per launch, about
constexpr int64_t WS_ROW_BYTES = 8ll * WS_MAXT * WS_BINS + 3 * 8 * WS_MAXT + 2 * 4 * WS_MAXT + 8;   // state of one pair
constexpr int WH_THREADS = 1024;
constexpr int64_t WH_CAP = 18432;      // 64-bit bins of a sweep: 144 KiB of LDS

static inline void reweight_path_count(int path) { count_path(PATHS_REWEIGHT, path); }   // enum gpemu_reweight_path

static __device__ __forceinline__ double rw_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---- log-ratio of a prior scenario ------------------------------------------------------------------------------------
struct LogPriorArgs {
  RowsView X;
  int R;
  const int *kind;          // [R][d]
  const double *a, *b;      // [R][d]
  double *L;
  int64_t ldl;
};

__global__ __launch_bounds__(256) void logprior_kernel(LogPriorArgs p) {
  __shared__ int s_kind[RW_MAX_R * RW_MAX_D];
  __shared__ double s_a[RW_MAX_R * RW_MAX_D], s_den[RW_MAX_R * RW_MAX_D];
  __shared__ int s_log[RW_MAX_D];     // does any scenario take the log of parameter i?
  const int tid = threadIdx.x, d = p.X.d, n = p.R * d;
  if (tid < RW_MAX_D) s_log[tid] = 0;
  __syncthreads();
  for (int t = tid; t < n; t += 256) {
    const int kd = p.kind[t];
    const double bb = p.b[t];
    s_kind[t] = kd;
    s_a[t] = p.a[t];
    s_den[t] = 2.0 * (bb * bb);        // one rounding: the doubling is exact
    if (kd == 1 || kd == 3) s_log[t % d] = 1;
  }
  __syncthreads();
  const int64_t s = (int64_t)blockIdx.x * 256 + tid;
  if (s >= p.X.rows()) return;
  const double *row = p.X.row(s);
  double x[RW_MAX_D], lx[RW_MAX_D];
#pragma unroll
  for (int i = 0; i < RW_MAX_D; ++i) {
    x[i] = i < d ? row[i] : 1.0;
    lx[i] = (i < d && s_log[i]) ? log(x[i]) : 0.0;
  }
  for (int r = 0; r < p.R; ++r) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < RW_MAX_D; ++i) {
      if (i < d) {
        const int kd = s_kind[r * d + i];
        double f = 0.0;
        if (kd == 1) {
          f = -lx[i];
        } else if (kd == 2) {
          const double t = x[i] - s_a[r * d + i];
          f = -((t * t) / s_den[r * d + i]);
        } else if (kd == 3) {
          const double t = lx[i] - s_a[r * d + i];
          f = -lx[i] - (t * t) / s_den[r * d + i];
        }
        acc = i == 0 ? f : acc + f;
      }
    }
    p.L[(int64_t)r * p.ldl + s] = acc;
  }
}

static int logprior_check(int d, int R, const int *kind, const double *a, const double *b, const double *lower) {
  GP_ARG(d >= 1 && d <= RW_MAX_D, "d must be in [1, 16]");
  GP_ARG(R >= 1 && R <= RW_MAX_R, "R must be in [1, 64]");
  GP_ARG(kind && a && b && lower, "null pointer");
  for (int i = 0; i < d; ++i) GP_ARG(std::isfinite(lower[i]), "every lower bound must be finite");
  for (int t = 0; t < R * d; ++t) {
    GP_ARG(kind[t] >= 0 && kind[t] <= 3, "kind must be 0 (flat), 1 (log-uniform), 2 (normal) or 3 (log-normal)");
    if (kind[t] == 1 || kind[t] == 3) GP_ARG(lower[t % d] > 0.0, "a log-uniform or log-normal prior needs a lower bound > 0");
    if (kind[t] >= 2) GP_ARG(std::isfinite(a[t]) && std::isfinite(b[t]) && b[t] > 0.0, "a must be finite, b finite and > 0");
  }
  return GPEMU_OK;
}

static int logprior_rows(const RowsView &X, int R, const int *kind, const double *a, const double *b, double *dL,
                         int64_t ldl, hipStream_t st) {
  const int64_t n = (int64_t)R * X.d;
  DevScope sc(st);
  LogPriorArgs p;
  int *dk = nullptr;
  double *da = nullptr, *db = nullptr;
  GP_TRY(sc.alloc(&dk, n));
  GP_TRY(sc.alloc(&da, n));
  GP_TRY(sc.alloc(&db, n));
  GP_TRY(upload(dk, kind, n, st));
  GP_TRY(upload(da, a, n, st));
  GP_TRY(upload(db, b, n, st));
  p.X = X; p.R = R; p.kind = dk; p.a = da; p.b = db; p.L = dL; p.ldl = ldl;
  reweight_path_count(GPEMU_REWEIGHT_PATH_LOGPRIOR);
  hipLaunchKernelGGL(logprior_kernel, dim3((unsigned)((X.rows() + 255) / 256)), dim3(256), 0, st, p);
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(st));   // the tables are read by the copies above
  return GPEMU_OK;
}

// the rows of the _dev calls as a view, within these calls' limits
static int reweight_view(const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows, int d,
                         RowsView *v) {
  GP_ARG(d >= 1 && d <= RW_MAX_D, "d must be in [1, 16]");
  *v = RowsView{dX, n_blocks, block_rows, block_stride_rows * d, d};
  GP_TRY(rows_check(*v));
  GP_ARG(n_blocks <= ((1ll << 31) - 1) / block_rows, "S = n_blocks * block_rows must be below 2^31");
  return GPEMU_OK;
}

// ---- log-sum-exp of rows ----------------------------------------------------------------------------------------------
// part[r nchunk + c] = the maximum of chunk c of row r; workgroup (c, r)
__global__ __launch_bounds__(256) void lse_max_kernel(const double *__restrict__ L, int64_t ldl, int64_t S,
                                                      int64_t nchunk, double *__restrict__ part) {
  __shared__ double ws[4];
  const int64_t c = blockIdx.x, r = blockIdx.y;
  double m = -INFINITY;
  bool nan = false;
  for (int j = 0; j < RW_SUM / 256; ++j) {
    const int64_t i = c * RW_SUM + (int64_t)j * 256 + threadIdx.x;
    if (i < S) {
      const double v = L[r * ldl + i];
      nan |= (v != v);
      m = fmax(m, v);
    }
  }
  if (nan) m = INFINITY;   // fmax drops a NaN: +inf makes the row's result NaN below (inf - inf)
  m = wg_max_b<4>(m, ws);
  if (threadIdx.x == 0) part[r * nchunk + c] = m;
}

// mx[r] = the maximum of the row's chunk maxima; one thread per row
__global__ __launch_bounds__(256) void lse_max_finish_kernel(const double *__restrict__ part, int64_t R, int64_t nchunk,
                                                             double *__restrict__ mx) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  double m = -INFINITY;
  for (int64_t c = 0; c < nchunk; ++c) m = fmax(m, part[r * nchunk + c]);
  mx[r] = m;
}

// part[r nchunk + c] = sum over chunk c of exp(L - mx[r]); workgroup (c, r)
__global__ __launch_bounds__(256) void lse_sum_kernel(const double *__restrict__ L, int64_t ldl, int64_t S,
                                                      int64_t nchunk, const double *__restrict__ mx,
                                                      double *__restrict__ part) {
  __shared__ double ws[4];
  const int64_t c = blockIdx.x, r = blockIdx.y;
  const double m = mx[r];
  double acc = 0.0;
  for (int j = 0; j < RW_SUM / 256; ++j) {
    const int64_t i = c * RW_SUM + (int64_t)j * 256 + threadIdx.x;
    if (i < S) acc += exp(L[r * ldl + i] - m);
  }
  acc = wg_sum_b<4>(acc, ws);
  if (threadIdx.x == 0) part[r * nchunk + c] = acc;
}

// lse[r] = mx[r] + log(the chunk sums added in chunk order); lme[r] = lse[r] - log S; one thread per row
__global__ __launch_bounds__(256) void lse_finish_kernel(const double *__restrict__ part, int64_t R, int64_t nchunk,
                                                         const double *__restrict__ mx, double log_s,
                                                         double *__restrict__ lse, double *__restrict__ lme) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  double acc = 0.0;
  for (int64_t c = 0; c < nchunk; ++c) acc += part[r * nchunk + c];
  const double m = mx[r];
  const double v = (m == -INFINITY) ? -INFINITY : m + log(acc);   // a row of -inf: log-sum-exp -inf, no NaN from inf - inf
  lse[r] = v;
  if (lme) lme[r] = v - log_s;
}

// lw[r S + i] = L[r ldl + i] - lse[r]
__global__ __launch_bounds__(256) void lse_normalise_kernel(const double *__restrict__ L, int64_t ldl, int64_t S,
                                                            const double *__restrict__ lse, double *__restrict__ lw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (i < S) lw[r * S + i] = L[r * ldl + i] - lse[r];
}

static int logmeanexp_rows(int64_t R, int64_t S, const double *dL, int64_t ldl, double *dlme, double *dlw,
                           hipStream_t st) {
  const int64_t nchunk = (S + RW_SUM - 1) / RW_SUM;
  DevScope sc(st);
  double *part = nullptr, *mx = nullptr, *lse = nullptr;
  GP_TRY(sc.alloc(&part, R * nchunk));
  GP_TRY(sc.alloc(&mx, R));
  GP_TRY(sc.alloc(&lse, R));
  const dim3 grid((unsigned)nchunk, (unsigned)R), fin((unsigned)((R + 255) / 256));
  reweight_path_count(GPEMU_REWEIGHT_PATH_LOGSUMEXP);
  hipLaunchKernelGGL(lse_max_kernel, grid, dim3(256), 0, st, dL, ldl, S, nchunk, part);
  hipLaunchKernelGGL(lse_max_finish_kernel, fin, dim3(256), 0, st, part, R, nchunk, mx);
  hipLaunchKernelGGL(lse_sum_kernel, grid, dim3(256), 0, st, dL, ldl, S, nchunk, mx, part);
  hipLaunchKernelGGL(lse_finish_kernel, fin, dim3(256), 0, st, part, R, nchunk, mx, std::log((double)S), lse, dlme);
  if (dlw)
    hipLaunchKernelGGL(lse_normalise_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)R), dim3(256), 0, st, dL, ldl, S,
                       lse, dlw);
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

// ---- fixed-point weights ----------------------------------------------------------------------------------------------
// q[r ldq + i] = (u64) rint(exp(lw[r ldw + i]) 2^52) (0 for a NaN or a negative product); Q[r] += the workgroup's sum
__global__ __launch_bounds__(256) void quantise_kernel(const double *__restrict__ lw, int64_t ldw, int64_t S,
                                                       u64 *__restrict__ q, int64_t ldq, u64 *__restrict__ Q) {
  __shared__ u64 red[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  u64 v = 0;
  if (i < S) {
    const double e = rint(exp(lw[r * ldw + i]) * 4503599627370496.0);
    v = (e >= 0.0 && e <= 9007199254740992.0) ? (u64)e : 0;
    q[r * ldq + i] = v;
  }
  const u64 s = wg_sum_a<256>(v, red);
  if (threadIdx.x == 0 && s) atomicAdd(&Q[r], s);
}

// ---- weighted selection -------------------------------------------------------------------------------------------------
struct WSelState {
  u64 *prefix = nullptr;    // [rows][WS_MAXT] key bits found so far, per target
  u64 *trem = nullptr;      // [rows][WS_MAXT] target within the weight of the elements that match the prefix, >= 1
  u64 *slotpre = nullptr;   // [rows][WS_MAXT] prefix of each slot
  int *slot = nullptr;      // [rows][WS_MAXT] slot of each target
  int *over = nullptr;      // [rows][WS_MAXT] the target is 0 or above the row's total weight
  int *nslot = nullptr;     // [rows]
  int *nan = nullptr;       // [rows] the value row holds a NaN
  u64 *hist = nullptr;      // [rows][WS_MAXT][WS_BINS] weight sums, zero between passes
};

// pair c0 + rl = (weight row w, value row v) = ((c0 + rl) / R_v, (c0 + rl) % R_v); targets: [R_w][nt_all] sorted per row
__global__ __launch_bounds__(256) void wsel_init_kernel(WSelState s, int rows, int nt, const u64 *__restrict__ targets,
                                                        int64_t nt_all, int64_t c0, int64_t R_v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * WS_MAXT) return;
  const int t = i % WS_MAXT, rl = i / WS_MAXT;
  const int64_t w = (c0 + rl) / R_v;
  const u64 tg = t < nt ? targets[w * nt_all + t] : 1;
  s.prefix[i] = 0;
  s.slotpre[i] = 0;
  s.trem[i] = tg;
  s.over[i] = tg == 0;
  s.slot[i] = 0;
  if (t == 0) {
    s.nslot[rl] = 1;
    s.nan[rl] = 0;
  }
}

// the sum of v over the lanes of the wave, in every lane
static __device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// workgroup (pair rl, slice c) of the batch: elements [c slice, (c + 1) slice) of the value row
__global__ __launch_bounds__(256) void wsel_hist_kernel(WSelState s, const double *__restrict__ V, int64_t row_stride,
                                                        int64_t elem_stride, int64_t S, const u64 *__restrict__ q,
                                                        int64_t ldq, int64_t c0, int64_t R_v, int nblk, int64_t slice,
                                                        int pass) {
  __shared__ u64 h[WS_MAXT * WS_BINS];
  __shared__ u64 spre[WS_MAXT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t rl = blockIdx.x / nblk, c = blockIdx.x % nblk;
  const int ns = s.nslot[rl];
  for (int t = tid; t < ns * WS_BINS; t += 256) h[t] = 0;
  if (tid < WS_MAXT) spre[tid] = s.slotpre[rl * WS_MAXT + tid];
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const int64_t w = (c0 + rl) / R_v, v = (c0 + rl) % R_v;
  const double *row = V + v * row_stride;
  const u64 *qrow = q + w * ldq;
  const int64_t base = c * slice, end = (base + slice < S) ? base + slice : S;
  bool seen_nan = false;
  for (int64_t off = base; off < end; off += 256) {   // the trip count is the same for every lane
    const int64_t i = off + tid;
    int bin = -1;
    u64 wt = 0;
    if (i < end) {
      const double x = row[i * elem_stride];
      const u64 key = sel_key(x);
      if (pass == 0) {
        bin = (int)(key >> 56);
        seen_nan |= (x != x);
      } else {
        const u64 hi = key >> (shift + 8);
        for (int j = 0; j < ns; ++j)
          if ((spre[j] >> (shift + 8)) == hi) bin = j * WS_BINS + (int)((key >> shift) & 255);
      }
      if (bin >= 0) {
        wt = qrow[i];
        if (wt == 0) bin = -1;
      }
    }
    // the lanes that agree with the wave's first lane add once: the leading bytes of real data are nearly constant
    const int lead = __builtin_amdgcn_readfirstlane(bin);
    const u64 led = wave_sum_u64(bin == lead ? wt : 0);
    if (lead >= 0 && lane == 0) atomicAdd(&h[lead], led);
    if (bin >= 0 && bin != lead) atomicAdd(&h[bin], wt);
  }
  __syncthreads();
  u64 *g = s.hist + rl * (WS_MAXT * WS_BINS);
  for (int t = tid; t < ns * WS_BINS; t += 256)
    if (h[t]) atomicAdd(&g[t], h[t]);
  if (seen_nan) s.nan[rl] = 1;
}

// one workgroup per pair: extend every target's prefix by the digit of this pass, regroup the slots, clear the histograms
__global__ __launch_bounds__(256) void wsel_scan_kernel(WSelState s, int nt, int pass) {
  __shared__ u64 sh[WS_MAXT * WS_BINS];
  __shared__ u64 pre[WS_MAXT];
  const int tid = threadIdx.x;
  const int64_t rl = blockIdx.x;
  const int ns = s.nslot[rl];
  u64 *g = s.hist + rl * (WS_MAXT * WS_BINS);
  for (int t = tid; t < ns * WS_BINS; t += 256) {
    sh[t] = g[t];
    g[t] = 0;
  }
  __syncthreads();
  const int shift = 56 - 8 * pass;
  if (tid < nt) {
    const int64_t i = rl * WS_MAXT + tid;
    const u64 *hs = sh + s.slot[i] * WS_BINS;
    const u64 t = s.trem[i];
    u64 below = 0;
    int digit = -1;
    for (int b = 0; b < WS_BINS; ++b) {
      const u64 wsum = hs[b];
      if (t <= below + wsum) { digit = b; break; }   // the first bin whose cumulative weight reaches the target
      below += wsum;
    }
    if (digit < 0) {   // above the total weight: no element answers
      s.over[i] = 1;
      digit = WS_BINS - 1;
      below = t - 1;
    }
    const u64 p = s.prefix[i] | ((u64)digit << shift);
    s.prefix[i] = p;
    s.trem[i] = t - below;   // the target within the bin: in [1, wsum]
    pre[tid] = p;
  }
  __syncthreads();
  if (tid == 0) {   // sorted targets: prefixes ascend, equal ones are neighbours
    int n = 0;
    for (int r = 0; r < nt; ++r) {
      if (r == 0 || pre[r] != pre[r - 1]) s.slotpre[rl * WS_MAXT + n++] = pre[r];
      s.slot[rl * WS_MAXT + r] = n - 1;
    }
    s.nslot[rl] = n;
  }
}

// out[(c0 + rl) nt_all + perm[w][t]] = the element found; perm: [R_w][nt_all], of this group's targets
__global__ __launch_bounds__(256) void wsel_out_kernel(WSelState s, int rows, int nt, const int *__restrict__ perm,
                                                       int64_t nt_all, int64_t c0, int64_t R_v,
                                                       double *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * nt) return;
  const int rl = i / nt, t = i % nt;
  const int64_t w = (c0 + rl) / R_v;
  const bool bad = s.nan[rl] || s.over[rl * WS_MAXT + t];
  out[(c0 + rl) * nt_all + perm[w * nt_all + t]] = bad ? rw_nan() : sel_value(s.prefix[rl * WS_MAXT + t]);
}

static int wsel_check(int64_t R_v, int64_t S, int64_t R_w, int64_t n_targets, const u64 *targets) {
  GP_ARG(R_v > 0 && R_w > 0, "R_v and R_w must be positive");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(R_v <= ((1ll << 31) - 1) / R_w, "R_v * R_w must be below 2^31");
  GP_ARG(n_targets > 0 && n_targets < (1ll << 24) && targets, "n_targets must be in [1, 2^24)");
  for (int64_t i = 0; i < R_w * n_targets; ++i)
    GP_ARG(targets[i] >= 1 && targets[i] <= (1ull << 53), "every target must be in [1, 2^53]");
  return GPEMU_OK;
}

// dout[(w R_v + v) n_targets + i] = the smallest element x of value row v with sum_{x_s <= x} q[w][s] >= targets[w][i];
// the pairs go through the state in batches that fit workspace_bytes; waits for st
static int wsel_rows(const double *dV, int64_t R_v, int64_t S, int64_t row_stride, int64_t elem_stride, int64_t R_w,
                     const u64 *dq, int64_t ldq, int64_t nt_all, const u64 *targets, double *dout,
                     int64_t workspace_bytes, hipStream_t st) {
  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t pairs = R_w * R_v;
  const int64_t rows_cap = std::min<int64_t>(std::min<int64_t>(pairs, WS_ROWS), budget / WS_ROW_BYTES);
  if (rows_cap < 1) {
    set_error("weighted_select: out of memory: the state of one (weight row, value row) pair needs %lld bytes; %lld bytes %s",
              (long long)WS_ROW_BYTES, (long long)budget, workspace_budget_name(workspace_bytes));
    return GPEMU_ERR_HIP;
  }
  // per weight row: the targets ascending, and where each goes in the caller's order
  std::vector<u64> sorted((size_t)(R_w * nt_all));
  std::vector<int> perm((size_t)(R_w * nt_all));
  for (int64_t w = 0; w < R_w; ++w) {
    int *o = perm.data() + w * nt_all;
    const u64 *tw = targets + w * nt_all;
    std::iota(o, o + nt_all, 0);
    std::stable_sort(o, o + nt_all, [&](int x, int y) { return tw[x] < tw[y]; });
    for (int64_t i = 0; i < nt_all; ++i) sorted[(size_t)(w * nt_all + i)] = tw[o[i]];
  }
  DevScope sc(st);
  WSelState s;
  u64 *dt = nullptr;
  int *dperm = nullptr;
  GP_TRY(sc.alloc(&s.prefix, rows_cap * WS_MAXT));
  GP_TRY(sc.alloc(&s.trem, rows_cap * WS_MAXT));
  GP_TRY(sc.alloc(&s.slotpre, rows_cap * WS_MAXT));
  GP_TRY(sc.alloc(&s.slot, rows_cap * WS_MAXT));
  GP_TRY(sc.alloc(&s.over, rows_cap * WS_MAXT));
  GP_TRY(sc.alloc(&s.nslot, rows_cap));
  GP_TRY(sc.alloc(&s.nan, rows_cap));
  GP_TRY(sc.alloc(&s.hist, rows_cap * WS_MAXT * WS_BINS));
  GP_TRY(sc.alloc(&dt, R_w * nt_all));
  GP_TRY(sc.alloc(&dperm, R_w * nt_all));
  GP_TRY(upload(dt, sorted.data(), R_w * nt_all, st));
  GP_TRY(upload(dperm, perm.data(), R_w * nt_all, st));
  GP_HIP(hipMemsetAsync(s.hist, 0, sizeof(u64) * (size_t)rows_cap * WS_MAXT * WS_BINS, st));

  for (int64_t c0 = 0; c0 < pairs; c0 += rows_cap) {
    const int rows = (int)std::min<int64_t>(rows_cap, pairs - c0);
    int64_t nblk = std::max<int64_t>(1, std::min((S + WS_SLICE - 1) / WS_SLICE, WS_MAX_WG / rows));
    const int64_t slice = round_up((S + nblk - 1) / nblk, 256);
    nblk = (S + slice - 1) / slice;
    for (int64_t g0 = 0; g0 < nt_all; g0 += WS_MAXT) {
      const int nt = (int)std::min<int64_t>(WS_MAXT, nt_all - g0);
      hipLaunchKernelGGL(wsel_init_kernel, dim3((unsigned)((rows * WS_MAXT + 255) / 256)), dim3(256), 0, st, s, rows, nt,
                         dt + g0, nt_all, c0, R_v);
      GP_HIP(hipGetLastError());
      for (int pass = 0; pass < WS_PASSES; ++pass) {
        reweight_path_count(GPEMU_REWEIGHT_PATH_WSEL_HIST_PASS);
        hipLaunchKernelGGL(wsel_hist_kernel, dim3((unsigned)(rows * nblk)), dim3(256), 0, st, s, dV, row_stride,
                           elem_stride, S, dq, ldq, c0, R_v, (int)nblk, slice, pass);
        GP_HIP(hipGetLastError());
        reweight_path_count(GPEMU_REWEIGHT_PATH_WSEL_SCAN);
        hipLaunchKernelGGL(wsel_scan_kernel, dim3((unsigned)rows), dim3(256), 0, st, s, nt, pass);
        GP_HIP(hipGetLastError());
      }
      hipLaunchKernelGGL(wsel_out_kernel, dim3((unsigned)((rows * nt + 255) / 256)), dim3(256), 0, st, s, rows, nt,
                         dperm + g0, nt_all, c0, R_v, dout);
      GP_HIP(hipGetLastError());
    }
  }
  GP_HIP(hipStreamSynchronize(st));   // `sorted` and `perm` are read by the copies above
  return GPEMU_OK;
}

// ---- weighted histograms ----------------------------------------------------------------------------------------------
struct WHistArgs {
  RowsView X;
  int64_t S, rows_per_wg;
  const u64 *q;                    // [R_w][ldq]
  int64_t ldq;
  const double *e1, *e2;           // [d][nb1 + 1], [d][nb2 + 1]
  int nb1, nb2;
  int a0, a1, p0, p1;              // this sweep: 1-D histograms of parameters [a0, a1), pairs [p0, p1)
  int i0, j0;                      // pair p0 = (i0, j0)
  int band0, band;                 // ... of the pairs, the bins [band0, band0 + band) of the first index
  u64 *hist1, *hist2;              // [R_w][d][nb1], [R_w][np][nb2][nb2]
  int64_t n1_all, n2_all;          // d nb1, np nb2^2
};

// gpemu_marginal_hist's rule (k_marginal.hip: mh_bin): the bin b with e[b] <= x < e[b + 1], the last one closed on the
// right; -1 outside [e[0], e[nb]] and for NaN.  tab = {e[0], e[nb], nb / (e[nb] - e[0])}
static __device__ __forceinline__ int wh_bin(double x, const double *__restrict__ e, int nb, const double *tab) {
  const double e0 = tab[0], eN = tab[1];
  if (!(x >= e0 && x <= eN)) return -1;
  double t = (x - e0) * tab[2];
  t = fmin(fmax(t, 0.0), (double)(nb - 1));   // a NaN guess (an infinite span) starts at 0
  int b = (int)t;
  while (b > 0 && x < e[b]) --b;
  while (b < nb - 1 && x >= e[b + 1]) ++b;
  return b;
}

template <int DP>
__global__ __launch_bounds__(WH_THREADS) void whist_kernel(WHistArgs a) {
  extern __shared__ u64 wh_lds[];              // the bins: 1-D section, then the pairs' bands
  __shared__ double tab[2][RW_MAX_D][3];
  const int tid = threadIdx.x;
  const int d = a.X.d, nb1 = a.nb1, nb2 = a.nb2, psz = a.band * nb2;
  const int n1 = (a.a1 - a.a0) * nb1, nbins = n1 + (a.p1 - a.p0) * psz;
  for (int w = tid; w < nbins; w += WH_THREADS) wh_lds[w] = 0;
  if (tid < 2 * d) {
    const int which = tid / d, k = tid % d, nb = which ? nb2 : nb1;
    const double *e = (which ? a.e2 : a.e1) + (int64_t)k * (nb + 1);
    tab[which][k][0] = e[0];
    tab[which][k][1] = e[nb];
    tab[which][k][2] = (double)nb / (e[nb] - e[0]);
  }
  __syncthreads();
  const u64 *qrow = a.q + (int64_t)blockIdx.y * a.ldq;
  const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_wg, r1 = (r0 + a.rows_per_wg < a.S) ? r0 + a.rows_per_wg : a.S;
  for (int64_t r = r0 + tid; r < r1; r += WH_THREADS) {
    const u64 wt = qrow[r];
    if (wt == 0) continue;
    const double *row = a.X.row(r);
    u64 pk[DP / 4];   // the 2-D bins + 1 (0: outside), 16 bits each: k is uniform, a select per word keeps them in registers
#pragma unroll
    for (int w = 0; w < DP / 4; ++w) pk[w] = 0;
#pragma unroll 1
    for (int k = 0; k < d; ++k) {
      const double xv = row[k];
      if (k >= a.a0 && k < a.a1) {
        const int b = wh_bin(xv, a.e1 + (int64_t)k * (nb1 + 1), nb1, tab[0][k]);
        if (b >= 0) atomicAdd(&wh_lds[(k - a.a0) * nb1 + b], wt);
      }
      if (a.p1 > a.p0) {
        const u64 b = (u64)(wh_bin(xv, a.e2 + (int64_t)k * (nb2 + 1), nb2, tab[1][k]) + 1) << ((k & 3) * 16);
#pragma unroll
        for (int w = 0; w < DP / 4; ++w) pk[w] |= (w == (k >> 2)) ? b : 0;
      }
    }
    if (a.p1 > a.p0) {
      int i = a.i0, j = a.j0, off = n1;   // pair p0 = (i0, j0), then row-major: the index is the same for every lane
#pragma unroll 1
      for (int p = a.p0; p < a.p1; ++p) {
        u64 wi = 0, wj = 0;
#pragma unroll
        for (int w = 0; w < DP / 4; ++w) {
          wi = (w == (i >> 2)) ? pk[w] : wi;
          wj = (w == (j >> 2)) ? pk[w] : wj;
        }
        int bi = (int)((wi >> ((i & 3) * 16)) & 0xffff) - 1;
        const int bj = (int)((wj >> ((j & 3) * 16)) & 0xffff) - 1;
        bi -= a.band0;
        if (bi >= 0 && bi < a.band && bj >= 0) atomicAdd(&wh_lds[off + bi * nb2 + bj], wt);
        off += psz;
        if (++j == d) {
          ++i;
          j = i + 1;
        }
      }
    }
  }
  __syncthreads();
  u64 *g1 = a.hist1 + (int64_t)blockIdx.y * a.n1_all + (int64_t)a.a0 * nb1;
  u64 *g2 = a.hist2 + (int64_t)blockIdx.y * a.n2_all;
  for (int w = tid; w < nbins; w += WH_THREADS) {
    const u64 v = wh_lds[w];
    if (!v) continue;
    if (w < n1) {
      atomicAdd(&g1[w], v);
    } else {
      const int pl = (w - n1) / psz, rem = (w - n1) % psz;
      atomicAdd(&g2[(int64_t)(a.p0 + pl) * nb2 * nb2 + (int64_t)a.band0 * nb2 + rem], v);
    }
  }
}

// w_inside[(w d + j)] = the sum of hist1[w][j][.]; workgroup w d + j
__global__ __launch_bounds__(256) void whist_inside_kernel(const u64 *__restrict__ hist1, int nb1,
                                                           u64 *__restrict__ w_inside) {
  __shared__ u64 red[256];
  u64 s = 0;
  for (int b = threadIdx.x; b < nb1; b += 256) s += hist1[(int64_t)blockIdx.x * nb1 + b];
  s = wg_sum_a<256>(s, red);
  if (threadIdx.x == 0) w_inside[blockIdx.x] = s;
}

struct WHistSweep { int a0, a1, p0, p1, band0, band; };

// the sweeps of one call; cap: 64-bit bins per sweep.  nb2^2 <= cap: floor(cap / nb2^2) whole pairs per sweep, the 1-D
// bins beside the last group where they fit, else in sweeps of their own (k_marginal.hip's plan); nb2^2 > cap: one pair
// per sweep, in bands of floor(cap / nb2) bins of its first index
static std::vector<WHistSweep> whist_plan(int d, int nb1, int nb2, int64_t cap) {
  std::vector<WHistSweep> plan;
  const int np = d * (d - 1) / 2;
  const int64_t sq = (int64_t)nb2 * nb2, dpg = cap / nb1;
  if (sq <= cap) {
    const int64_t ppg = cap / sq;
    for (int p0 = 0; p0 < np; p0 += (int)ppg) plan.push_back({0, 0, p0, (int)std::min<int64_t>(np, p0 + ppg), 0, nb2});
  } else {
    const int band = (int)(cap / nb2);
    for (int p = 0; p < np; ++p)
      for (int b0 = 0; b0 < nb2; b0 += band) plan.push_back({0, 0, p, p + 1, b0, std::min(band, nb2 - b0)});
  }
  int a = 0;
  if (!plan.empty()) {   // beside the last sweep of pairs, as many parameters as fit
    WHistSweep &last = plan.back();
    a = (int)std::min<int64_t>(d, (cap - (int64_t)(last.p1 - last.p0) * last.band * nb2) / nb1);
    last.a1 = a;
  }
  for (; a < d; a += (int)dpg) plan.push_back({a, (int)std::min<int64_t>(d, a + dpg), 0, 0, 0, nb2});
  return plan;
}

static int whist_check(int d, int64_t R_w, int nb1, const double *edges1, int nb2, const double *edges2,
                       int64_t group_bins, const void *hist1, const void *hist2, const void *w_inside1) {
  GP_ARG(d >= 1 && d <= RW_MAX_D, "d must be in [1, 16]");
  GP_ARG(R_w >= 1 && R_w <= 65535, "R_w must be in [1, 65535]");
  GP_ARG(nb1 >= 1 && nb1 <= 4096, "nb1 must be in [1, 4096]");
  GP_ARG(nb2 >= 1 && nb2 <= 256, "nb2 must be in [1, 256]");
  GP_ARG(edges1 && edges2 && hist1 && w_inside1 && (hist2 || d == 1), "null pointer");
  GP_ARG(group_bins == 0 || (group_bins >= std::max(nb1, nb2) && group_bins <= WH_CAP),
         "group_bins must be 0 or in [max(nb1, nb2), 18432]");
  for (int which = 0; which < 2; ++which) {
    const double *e = which ? edges2 : edges1;
    const int nb = which ? nb2 : nb1;
    for (int k = 0; k < d; ++k)
      for (int b = 0; b <= nb; ++b) {
        const double v = e[(int64_t)k * (nb + 1) + b];
        GP_ARG(std::isfinite(v), "bin edges must be finite");
        GP_ARG(b == 0 || v > e[(int64_t)k * (nb + 1) + b - 1], "bin edges must be strictly increasing");
      }
  }
  return GPEMU_OK;
}

// the sweeps over device rows; waits for st
static int whist_rows(const RowsView &X, int64_t R_w, const u64 *dq, int64_t ldq, int nb1, const double *edges1, int nb2,
                      const double *edges2, int64_t group_bins, u64 *dhist1, u64 *dhist2, u64 *dw_inside1,
                      hipStream_t st) {
  const int d = X.d;
  const int64_t S = X.rows(), np = d * (d - 1) / 2;
  const std::vector<WHistSweep> plan = whist_plan(d, nb1, nb2, group_bins ? group_bins : WH_CAP);
  DevScope sc(st);
  double *de1 = nullptr, *de2 = nullptr;
  GP_TRY(sc.alloc(&de1, (int64_t)d * (nb1 + 1)));
  GP_TRY(sc.alloc(&de2, (int64_t)d * (nb2 + 1)));
  GP_TRY(upload(de1, edges1, (int64_t)d * (nb1 + 1), st));
  GP_TRY(upload(de2, edges2, (int64_t)d * (nb2 + 1), st));
  WHistArgs a;
  a.X = X; a.S = S; a.q = dq; a.ldq = ldq;
  a.rows_per_wg = std::max<int64_t>(4096, round_up((S + 1023) / 1024, 256));
  a.e1 = de1; a.e2 = de2; a.nb1 = nb1; a.nb2 = nb2;
  a.hist1 = dhist1; a.hist2 = dhist2;
  a.n1_all = (int64_t)d * nb1; a.n2_all = np * nb2 * nb2;
  GP_HIP(hipMemsetAsync(dhist1, 0, sizeof(u64) * (size_t)(R_w * a.n1_all), st));
  if (np > 0) GP_HIP(hipMemsetAsync(dhist2, 0, sizeof(u64) * (size_t)(R_w * a.n2_all), st));
  const unsigned nwg = (unsigned)((S + a.rows_per_wg - 1) / a.rows_per_wg);
  const void *fn = d <= 8 ? (const void *)whist_kernel<8> : (const void *)whist_kernel<16>;
  GP_TRY(allow_dynamic_lds(fn, (int)(8 * WH_CAP)));
  for (const WHistSweep &sw : plan) {
    a.a0 = sw.a0; a.a1 = sw.a1; a.p0 = sw.p0; a.p1 = sw.p1; a.band0 = sw.band0; a.band = sw.band;
    int i0 = 0, rem = sw.p0;   // row i of the pair list holds d - 1 - i pairs
    while (i0 < d - 1 && rem >= d - 1 - i0) rem -= d - 1 - i0++;
    a.i0 = i0; a.j0 = i0 + 1 + rem;
    const int64_t nbins = (int64_t)(sw.a1 - sw.a0) * nb1 + (int64_t)(sw.p1 - sw.p0) * sw.band * nb2;
    const size_t lds = (size_t)(8 * std::max<int64_t>(nbins, 1));
    reweight_path_count(GPEMU_REWEIGHT_PATH_WHIST_SWEEP);
    if (sw.p1 > sw.p0) reweight_path_count(GPEMU_REWEIGHT_PATH_WHIST_PAIR_GROUP);
    if (d <= 8)
      hipLaunchKernelGGL(whist_kernel<8>, dim3(nwg, (unsigned)R_w), dim3(WH_THREADS), lds, st, a);
    else
      hipLaunchKernelGGL(whist_kernel<16>, dim3(nwg, (unsigned)R_w), dim3(WH_THREADS), lds, st, a);
    GP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(whist_inside_kernel, dim3((unsigned)(R_w * d)), dim3(256), 0, st, dhist1, nb1, dw_inside1);
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_reweight_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_REWEIGHT, out, n); }

int gpemu_logprior_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows,
                       int d, int R, const int *kind, const double *a, const double *b, const double *lower, double *dL,
                       int64_t ldl, void *stream) {
  GP_ARG(dX && dL, "null pointer");
  RowsView X;
  GP_TRY(reweight_view(dX, n_blocks, block_rows, block_stride_rows, d, &X));
  GP_TRY(logprior_check(d, R, kind, a, b, lower));
  GP_ARG(ldl >= X.rows(), "ldl must be at least the number of rows");
  GP_TRY(device_ready(device));
  return logprior_rows(X, R, kind, a, b, dL, ldl, (hipStream_t)stream);
}

int gpemu_logprior(int device, int64_t S, int d, const double *X, int R, const int *kind, const double *a,
                   const double *b, const double *lower, double *L) {
  GP_ARG(X && L, "null pointer");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_TRY(logprior_check(d, R, kind, a, b, lower));
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  DevScope sc(st);
  double *dX = nullptr, *dL = nullptr;
  GP_TRY(sc.alloc(&dX, S * d));
  GP_TRY(sc.alloc(&dL, (int64_t)R * S));
  GP_TRY(upload(dX, X, S * d, st));
  GP_TRY(logprior_rows(RowsView{dX, 1, S, S * d, d}, R, kind, a, b, dL, S, st));
  GP_TRY(sc.download(L, dL, (int64_t)R * S));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_logmeanexp_dev(int device, int64_t R, int64_t S, const double *dL, int64_t ldl, double *dlme, double *dlw,
                         void *stream) {
  GP_ARG(dL && (dlme || dlw), "null pointer");
  GP_ARG(R >= 1 && R <= 65535, "R must be in [1, 65535]");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(ldl >= S, "ldl must be at least S");
  GP_TRY(device_ready(device));
  return logmeanexp_rows(R, S, dL, ldl, dlme, dlw, (hipStream_t)stream);
}

int gpemu_weights_fixed_dev(int device, int64_t R, int64_t S, const double *dlw, int64_t ldw, uint64_t *dq, int64_t ldq,
                            uint64_t *dQ, void *stream) {
  GP_ARG(dlw && dq && dQ, "null pointer");
  GP_ARG(R >= 1 && R <= 65535, "R must be in [1, 65535]");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(ldw >= S && ldq >= S, "the leading dimensions must be at least S");
  GP_TRY(device_ready(device));
  hipStream_t st = (hipStream_t)stream;
  GP_HIP(hipMemsetAsync(dQ, 0, sizeof(u64) * (size_t)R, st));
  reweight_path_count(GPEMU_REWEIGHT_PATH_QUANTISE);
  hipLaunchKernelGGL(quantise_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)R), dim3(256), 0, st, dlw, ldw, S,
                     (u64 *)dq, ldq, (u64 *)dQ);
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_weighted_select_dev(int device, int64_t R_v, int64_t S, const double *dV, int64_t row_stride,
                              int64_t elem_stride, int64_t R_w, const uint64_t *dq, int64_t ldq, int64_t n_targets,
                              const uint64_t *targets, double *dout, int64_t workspace_bytes, void *stream) {
  GP_ARG(dV && dq && dout, "null pointer");
  GP_TRY(wsel_check(R_v, S, R_w, n_targets, (const u64 *)targets));
  GP_ARG(row_stride > 0 && elem_stride > 0, "strides must be positive");
  GP_ARG(ldq >= S, "ldq must be at least S");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_TRY(device_ready(device));
  return wsel_rows(dV, R_v, S, row_stride, elem_stride, R_w, (const u64 *)dq, ldq, n_targets, (const u64 *)targets, dout,
                   workspace_bytes, (hipStream_t)stream);
}

int gpemu_weighted_select(int device, int64_t R_v, int64_t S, const double *V, int64_t R_w, const uint64_t *q,
                          int64_t n_targets, const uint64_t *targets, double *out) {
  GP_ARG(V && q && out, "null pointer");
  GP_TRY(wsel_check(R_v, S, R_w, n_targets, (const u64 *)targets));
  GP_ARG(R_v <= INT64_MAX / 8 / S && R_w <= INT64_MAX / 8 / S, "R * S overflows");
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  DevScope sc(st);
  double *dV = nullptr, *dout = nullptr;
  u64 *dq = nullptr;
  GP_TRY(sc.alloc(&dV, R_v * S));
  GP_TRY(sc.alloc(&dq, R_w * S));
  GP_TRY(sc.alloc(&dout, R_w * R_v * n_targets));
  GP_TRY(upload(dV, V, R_v * S, st));
  GP_TRY(upload(dq, (const u64 *)q, R_w * S, st));
  GP_TRY(wsel_rows(dV, R_v, S, S, 1, R_w, dq, S, n_targets, (const u64 *)targets, dout, 0, st));
  GP_TRY(sc.download(out, dout, R_w * R_v * n_targets));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_weighted_hist_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows,
                            int64_t block_stride_rows, int d, int64_t R_w, const uint64_t *dq, int64_t ldq, int nb1,
                            const double *edges1, int nb2, const double *edges2, int64_t group_bins, uint64_t *dhist1,
                            uint64_t *dhist2, uint64_t *dw_inside1, void *stream) {
  GP_ARG(dX && dq, "null pointer");
  RowsView X;
  GP_TRY(reweight_view(dX, n_blocks, block_rows, block_stride_rows, d, &X));
  GP_TRY(whist_check(d, R_w, nb1, edges1, nb2, edges2, group_bins, dhist1, dhist2, dw_inside1));
  GP_ARG(ldq >= X.rows(), "ldq must be at least the number of rows");
  GP_TRY(device_ready(device));
  return whist_rows(X, R_w, (const u64 *)dq, ldq, nb1, edges1, nb2, edges2, group_bins, (u64 *)dhist1, (u64 *)dhist2,
                    (u64 *)dw_inside1, (hipStream_t)stream);
}

int gpemu_weighted_hist(int device, int64_t S, int d, const double *X, int64_t R_w, const uint64_t *q, int nb1,
                        const double *edges1, int nb2, const double *edges2, int64_t group_bins, uint64_t *hist1,
                        uint64_t *hist2, uint64_t *w_inside1) {
  GP_ARG(X && q, "null pointer");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_TRY(whist_check(d, R_w, nb1, edges1, nb2, edges2, group_bins, hist1, hist2, w_inside1));
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  const int64_t np = d * (d - 1) / 2, n1 = R_w * d * nb1, n2 = R_w * np * nb2 * nb2;
  DevScope sc(st);
  double *dX = nullptr;
  u64 *dq = nullptr, *dh1 = nullptr, *dh2 = nullptr, *dwi = nullptr;
  GP_TRY(sc.alloc(&dX, S * d));
  GP_TRY(sc.alloc(&dq, R_w * S));
  GP_TRY(sc.alloc(&dh1, n1));
  GP_TRY(sc.alloc(&dh2, n2));
  GP_TRY(sc.alloc(&dwi, R_w * d));
  GP_TRY(upload(dX, X, S * d, st));
  GP_TRY(upload(dq, (const u64 *)q, R_w * S, st));
  GP_TRY(whist_rows(RowsView{dX, 1, S, S * d, d}, R_w, dq, S, nb1, edges1, nb2, edges2, group_bins, dh1, dh2, dwi, st));
  GP_TRY(sc.download((u64 *)hist1, dh1, n1));
  if (n2 > 0) GP_TRY(sc.download((u64 *)hist2, dh2, n2));
  GP_TRY(sc.download((u64 *)w_inside1, dwi, R_w * d));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

}  // extern "C"
