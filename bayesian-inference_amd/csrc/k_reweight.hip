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
// The weighted summaries are the shared ones (rows_dev.h) with the fixed-point weights q:
// gpemu_weighted_select* runs the radix select of k_select.hip (select_rows) on (weight row, value row) pairs,
// gpemu_weighted_hist* the histogram sweep of k_marginal.hip (hist_rows) with 64-bit bins, grid.y = the weight row.
// Only their checks, the select's budget rule and the path counters are here.
// Every weight is an integer and every sum of a row's weights is below 2^53: no result depends on the order of the
// atomics, on the grid, on the batches or on the run.  No floating-point atomics.
#include <algorithm>
#include <cmath>
#include <vector>

#include "internal.h"
#include "rows_dev.h"
#include "sampler_internal.h"
#include "wg_dev.h"

namespace gpemu {

constexpr int RW_MAX_D = ROWS_MAX_D;
constexpr int RW_MAX_R = 64;           // scenarios per logprior call
constexpr int64_t RW_SUM = 4096;       // samples per partial sum

static inline void reweight_path_count(int path) { count_path(PATHS_REWEIGHT, path); }   // enum gpemu_reweight_path

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
static int wsel_check(int64_t R_v, int64_t S, int64_t R_w, int64_t n_targets, const u64 *targets) {
  GP_ARG(R_v > 0 && R_w > 0, "R_v and R_w must be positive");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(R_v <= ((1ll << 31) - 1) / R_w, "R_v * R_w must be below 2^31");
  GP_ARG(n_targets > 0 && n_targets < (1ll << 24) && targets, "n_targets must be in [1, 2^24)");
  for (int64_t i = 0; i < R_w * n_targets; ++i)
    GP_ARG(targets[i] >= 1 && targets[i] <= (1ull << 53), "every target must be in [1, 2^53]");
  return GPEMU_OK;
}

// select_rows (rows_dev.h) with the weights dq, the pairs in batches that fit workspace_bytes; waits for st
static int wsel_rows(const double *dV, int64_t R_v, int64_t S, int64_t row_stride, int64_t elem_stride, int64_t R_w,
                     const u64 *dq, int64_t ldq, int64_t nt_all, const u64 *targets, double *dout,
                     int64_t workspace_bytes, hipStream_t st) {
  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t rows_cap = std::min<int64_t>(std::min<int64_t>(R_w * R_v, SEL_ROWS), budget / SEL_ROW_BYTES);
  if (rows_cap < 1) {
    set_error("weighted_select: out of memory: the state of one (weight row, value row) pair needs %lld bytes; %lld bytes %s",
              (long long)SEL_ROW_BYTES, (long long)budget, workspace_budget_name(workspace_bytes));
    return GPEMU_ERR_HIP;
  }
  return select_rows(dV, R_v, S, row_stride, elem_stride, R_w, dq, ldq, nt_all, targets, dout, rows_cap, [] {
    reweight_path_count(GPEMU_REWEIGHT_PATH_WSEL_HIST_PASS);
    reweight_path_count(GPEMU_REWEIGHT_PATH_WSEL_SCAN);
  }, st);
}

// ---- weighted histograms ----------------------------------------------------------------------------------------------
static int whist_check(int d, int64_t R_w, int nb1, const double *edges1, int nb2, const double *edges2,
                       int64_t group_bins, const void *hist1, const void *hist2, const void *w_inside1) {
  GP_ARG(d >= 1 && d <= RW_MAX_D, "d must be in [1, 16]");
  GP_ARG(R_w >= 1 && R_w <= 65535, "R_w must be in [1, 65535]");
  GP_ARG(nb1 >= 1 && nb1 <= 4096, "nb1 must be in [1, 4096]");
  GP_ARG(nb2 >= 1 && nb2 <= 256, "nb2 must be in [1, 256]");
  GP_ARG(edges1 && edges2 && hist1 && w_inside1 && (hist2 || d == 1), "null pointer");
  GP_ARG(group_bins == 0 || (group_bins >= std::max(nb1, nb2) && group_bins <= HIST_CAP64),
         "group_bins must be 0 or in [max(nb1, nb2), 18432]");
  GP_TRY(edges_check(edges1, d, nb1));
  GP_TRY(edges_check(edges2, d, nb2));
  return GPEMU_OK;
}

// hist_rows (rows_dev.h) with the weights dq; waits for st
static int whist_rows(const RowsView &X, int64_t R_w, const u64 *dq, int64_t ldq, int nb1, const double *edges1, int nb2,
                      const double *edges2, int64_t group_bins, u64 *dhist1, u64 *dhist2, u64 *dw_inside1,
                      hipStream_t st) {
  return hist_rows(X, R_w, dq, ldq, nb1, edges1, nb2, edges2, group_bins ? group_bins : HIST_CAP64, dhist1, dhist2,
                   dw_inside1, [](bool pairs) {
                     reweight_path_count(GPEMU_REWEIGHT_PATH_WHIST_SWEEP);
                     if (pairs) reweight_path_count(GPEMU_REWEIGHT_PATH_WHIST_PAIR_GROUP);
                   }, st);
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
  GP_TRY(rows_view(dX, n_blocks, block_rows, block_stride_rows, d, &X));
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
  GP_TRY(rows_view(dX, n_blocks, block_rows, block_stride_rows, d, &X));
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
