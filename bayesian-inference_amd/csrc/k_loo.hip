// Per-observable log-likelihoods of a stored chain and what is built on them (gpemu_loglik_pointwise*, gpemu_psis*,
// gpemu_weighted_moments_dev, gpemu_loo_group_rows_dev): Pareto-smoothed importance-sampling leave-one-out
// (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024), WAIC and the leave-one-observable-out moments
// of the parameters.
//
// Terms: the merged covariance keeps only the within-observable blocks (ref: emulation.py:370-388), so a group's
// log-likelihood is a sum of per-observable terms; T[o][s] is the term of block o for row s, in gpemu_logpost's
// normalisation.  PC means / variances come from gpemu_gp_predict_dev in fixed chunks of LOO_CHUNK logical rows (a chunk
// that is not contiguous in the caller's block layout is gathered first: k_postpred.hip's rule), then
//   loo_terms_kernel   one wave per (row, block): the likelihood's own block term (loglik_dev.h), lowrank_block_term<KMAX>
//                      (k <= 32) or lowrank_block_term_lds (33 <= k <= 64).  No prior box: a likelihood.
//
// PSIS of rows V[R][S] of log-likelihoods, per row: x_s = -V_s - max(-V) = min(V) - V_s (the same rounding), so the
// ascending order statistics of x are min(V) - (the descending ones of V): the row itself is sorted (k_rows.hip's radix
// sort, nothing else) and x_(i) is formed on the fly from the sorted keys -- monotone, ties in x contiguous.
//   psis_tail_kernel     cutoff x_c = max(x_(S-M-1), log DBL_MIN), tail = the n elements strictly above (binary search)
//   psis_gpd_k_kernel    workgroup (grid point j, row): b_j, k_j = mean log1p(-b_j t_i), L_j  (Zhang & Stephens 2009)
//   psis_gpd_fit_kernel  workgroup per row: the weights of the grid points, b-bar, k, sigma, k-hat
//   psis_smooth_kernel   the smoothed tail, psis_ties_kernel: tied raw values share the mean of their positions' values
//   psis_max_kernel / psis_sum_kernel / psis_var_kernel with their finish kernels: the log-sum-exps, the weights' ESS, the
//                        mean and the variance of V and, on request, the normalised log-weights in the input's order (the
//                        rank of a tail element: binary search in the sorted tail).
// Every sum over samples runs over chunks of LOO_SUM = 4096 fixed by the logical index: a lane adds its 16 elements in
// index order, then tree B of wg_dev.h, the chunks in order.  No floating-point atomics: no result bit
// depends on the grid, on the batches of rows that fit the workspace or on the run.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "internal.h"
#include "loglik_dev.h"
#include "rows_dev.h"
#include "sampler_internal.h"
#include "wg_dev.h"

namespace gpemu {

constexpr int64_t LOO_CHUNK = 2048;   // logical rows per predict pass (one pass of gpemu_gp_predict_dev)
constexpr int64_t LOO_SUM = 4096;     // samples per partial sum
constexpr int LOO_MAX_M = 512;        // grid points of the GPD fit: 30 + floor(sqrt(n)), n <= 3 sqrt(2^31)
constexpr int LOO_NSUM = 5;           // partial sums of the main pass
constexpr int LOO_STATE = 16;         // doubles of per-row state
enum { LS_VMIN = 0, LS_VMAX, LS_XC, LS_EXC, LS_KHAT, LS_SIGMA, LS_MXW, LS_MXE, LS_LSEW, LS_A, LS_Q, LS_B, LS_MEANV, LS_E };

static inline void loo_path_count(int path) { count_path(PATHS_LOO, path); }   // enum gpemu_loo_path

static __device__ __forceinline__ double loo_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---- the terms -------------------------------------------------------------------------------------------------------
struct TermArgs {
  RowsView X;                  // the caller's rows: a non-finite coordinate gives NaN terms
  int64_t r0, nb;              // this chunk: logical rows [r0, r0 + nb)
  const double *mean, *var;    // [nb][k] of the chunk
  const double *G, *g0, *scal; // the chain's constants
  int k, nblk;
  double *T;
  int64_t ldt;
};

// task t = o nb + s of the chunk on a wave of its own, four to a workgroup; KMAX = 0: the LDS form
template <int KMAX>
__global__ __launch_bounds__(256) void loo_terms_kernel(TermArgs a) {
  extern __shared__ __attribute__((aligned(16))) double loo_smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.x * 4 + wave;
  if (t >= a.nb * a.nblk) return;   // the whole wave; no workgroup barrier below
  const int o = (int)(t / a.nb);
  const int64_t s = t % a.nb;
  const int k = a.k;
  bool fin = true;
  if (lane < a.X.d) fin = isfinite(a.X.row(a.r0 + s)[lane]);
  double mu = 0.0, sd = 0.0;
  if (lane < k) {
    mu = a.mean[s * k + lane];
    double v = a.var[s * k + lane];
    if (v < 0.0) v = 0.0;
    sd = sqrt(v);
  }
  const double *Go = a.G + (int64_t)o * k * k, *g0o = a.g0 + (int64_t)o * k, *sco = a.scal + 2 * o;
  double term;
  if constexpr (KMAX == 0)   // 33 <= k <= 64: the k x k matrix in the wave's LDS
    term = lowrank_block_term_lds(Go, g0o, sco, k, mu, sd, lane, loo_smem + (size_t)wave * k * (k + 1), k + 1);
  else                       // block o's constants as "block 0" of lowrank_block_term (k_loglik.hip: task_term)
    term = lowrank_block_term<KMAX>(0, mu, sd, prefetch_block<KMAX>(Go, g0o, sco, k, lane), Go, g0o, sco, k, lane);
  if (!__all(fin)) term = loo_nan();
  if (lane == 0) a.T[(int64_t)o * a.ldt + a.r0 + s] = term;
}

static int launch_loo_terms(const TermArgs &a, hipStream_t st) {
  const int k = a.k;
  const dim3 grid((unsigned)((a.nb * a.nblk + 3) / 4)), block(256);
  if (k <= 32) {
    with_kmax(k, [&](auto km) { hipLaunchKernelGGL(loo_terms_kernel<decltype(km)::value>, grid, block, 0, st, a); });
  } else {
    const size_t shm = sizeof(double) * 4 * (size_t)k * (k + 1);
    if (shm > 64 * 1024) GP_TRY(allow_dynamic_lds((const void *)loo_terms_kernel<0>, (int)(sizeof(double) * 4 * 64 * 65)));
    hipLaunchKernelGGL(loo_terms_kernel<0>, grid, block, shm, st, a);
  }
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

// ---- sums in tree B (wg_dev.h) -------------------------------------------------------------------------------------
// the sum of f(i), i < n, by the whole workgroup (256 threads), in every thread: chunks of LOO_SUM in order, within a chunk
// every lane its 16 elements in index order, then tree B.  ws: 4 doubles of LDS
template <class F>
static __device__ __forceinline__ double loo_wg_sum(int64_t n, F f, double *ws) {
  const int tid = threadIdx.x;
  double total = 0.0;
  for (int64_t c0 = 0; c0 < n; c0 += LOO_SUM) {
    double acc = 0.0;
    for (int j = 0; j < LOO_SUM / 256; ++j) {
      const int64_t i = c0 + (int64_t)j * 256 + tid;
      if (i < n) acc += f(i);
    }
    total += wg_sum_b<4>(acc, ws);
  }
  return total;
}

// ---- PSIS ------------------------------------------------------------------------------------------------------------
struct PsisArgs {
  const double *V;             // element j of row r at V[r rs + j es]
  int64_t rs, es, S, row0;
  int rows;
  const u64 *sorted;           // [rows][S] the sorted keys of V
  int *nan;                    // [rows] the row holds a NaN (the sort) or an infinity (psis_tail_kernel)
  const int64_t *M;            // [R] tail sizes asked for
  int64_t Mmax, nchunk;
  double log_tiny;             // log(DBL_MIN)
  double *state;               // [rows][LOO_STATE]
  long long *nt;               // [rows] tail lengths
  double *gb, *gL;             // [rows][LOO_MAX_M] the GPD fit's grid
  double *smraw, *smt;         // [rows][Mmax] smoothed tail before / after the tie rule
  double *part;                // [rows][nchunk][LOO_NSUM]
  double *out;                 // [R][GPEMU_PSIS_NOUT]
  double *logw;                // [R][S] or null
};

// ascending order statistic i of x = min(V) - V
static __device__ __forceinline__ double psis_x(const u64 *k, int64_t S, double vmin, int64_t i) {
  return vmin - sel_value(k[S - 1 - i]);
}

// the first position in [lo, hi) of the ascending x whose element is > v (upper) or >= v (lower); hi if none
static __device__ __forceinline__ int64_t psis_bound(const u64 *k, int64_t S, double vmin, int64_t lo, int64_t hi, double v,
                                                     bool upper) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const double x = psis_x(k, S, vmin, mid);
    if (upper ? (x > v) : (x >= v)) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void psis_tail_kernel(PsisArgs a) {
  const int rl = blockIdx.x * 256 + threadIdx.x;
  if (rl >= a.rows) return;
  const u64 *k = a.sorted + (int64_t)rl * a.S;
  const int64_t S = a.S, M = a.M[a.row0 + rl];
  const double vmin = sel_value(k[0]), vmax = sel_value(k[S - 1]);
  const int64_t ic = (S - M - 1 > 0) ? S - M - 1 : 0;
  double xc = psis_x(k, S, vmin, ic);
  if (xc < a.log_tiny) xc = a.log_tiny;
  int64_t n = S - psis_bound(k, S, vmin, 0, S, xc, true);
  if (n > M) n = M;           // (cannot be for finite rows: the elements above x_(S-M-1) are at most M)
  if (isinf(vmin) || isinf(vmax)) a.nan[rl] = 1;   // x = min(V) - V is undefined: as a row with a NaN
  if (a.nan[rl]) n = 0;
  double *st = a.state + (int64_t)rl * LOO_STATE;
  st[LS_VMIN] = vmin;
  st[LS_VMAX] = vmax;
  st[LS_XC] = xc;
  st[LS_EXC] = exp(xc);
  st[LS_KHAT] = INFINITY;
  st[LS_SIGMA] = 0.0;
  a.nt[rl] = n;
}

// t_i = exp(x_(S - n + i)) - exp(x_c), i < n
static __device__ __forceinline__ double psis_t(const u64 *k, int64_t S, double vmin, int64_t n, double exc, int64_t i) {
  return exp(psis_x(k, S, vmin, S - n + i)) - exc;
}

__global__ __launch_bounds__(256) void psis_gpd_k_kernel(PsisArgs a) {
  __shared__ double ws[4];
  const int rl = blockIdx.y, j = blockIdx.x;
  const int64_t n = a.nt[rl], S = a.S;
  if (n <= 4) return;
  const int m = 30 + (int)floor(sqrt((double)n));
  if (j >= m) return;
  const u64 *k = a.sorted + (int64_t)rl * S;
  const double *st = a.state + (int64_t)rl * LOO_STATE;
  const double vmin = st[LS_VMIN], exc = st[LS_EXC];
  const int64_t iq = (int64_t)((double)n / 4.0 + 0.5) - 1;
  const double tq = psis_t(k, S, vmin, n, exc, iq), tn = psis_t(k, S, vmin, n, exc, n - 1);
  const double b = (1.0 - sqrt((double)m / ((double)(j + 1) - 0.5))) / (3.0 * tq) + 1.0 / tn;
  const double kj = loo_wg_sum(n, [&](int64_t i) { return log1p(-b * psis_t(k, S, vmin, n, exc, i)); }, ws) / (double)n;
  if (threadIdx.x == 0) {
    a.gb[rl * LOO_MAX_M + j] = b;
    a.gL[rl * LOO_MAX_M + j] = (double)n * (log(-(b / kj)) - kj - 1.0);
  }
}

__global__ __launch_bounds__(256) void psis_gpd_fit_kernel(PsisArgs a) {
  __shared__ double ws[4];
  __shared__ double sL[LOO_MAX_M], sb[LOO_MAX_M], sw[LOO_MAX_M];
  __shared__ double s_bbar;
  const int rl = blockIdx.x, tid = threadIdx.x;
  const int64_t n = a.nt[rl], S = a.S;
  if (n <= 4) return;
  const int m = 30 + (int)floor(sqrt((double)n));
  for (int j = tid; j < m; j += 256) {
    sL[j] = a.gL[rl * LOO_MAX_M + j];
    sb[j] = a.gb[rl * LOO_MAX_M + j];
  }
  __syncthreads();
  for (int j = tid; j < m; j += 256) {
    double acc = 0.0;
    for (int i = 0; i < m; ++i) acc += exp(sL[i] - sL[j]);
    sw[j] = 1.0 / acc;   // an overflow of the sum: weight 0
  }
  __syncthreads();
  if (tid == 0) {
    const double thr = 10.0 * DBL_EPSILON;
    double tot = 0.0;
    for (int j = 0; j < m; ++j)
      if (sw[j] >= thr) tot += sw[j];
    double bb = 0.0;
    for (int j = 0; j < m; ++j)
      if (sw[j] >= thr) bb += sb[j] * (sw[j] / tot);
    s_bbar = bb;
  }
  __syncthreads();
  const double bbar = s_bbar;
  const u64 *k = a.sorted + (int64_t)rl * S;
  double *st = a.state + (int64_t)rl * LOO_STATE;
  const double vmin = st[LS_VMIN], exc = st[LS_EXC];
  const double kk = loo_wg_sum(n, [&](int64_t i) { return log1p(-bbar * psis_t(k, S, vmin, n, exc, i)); }, ws) / (double)n;
  if (tid == 0) {
    st[LS_SIGMA] = -kk / bbar;
    st[LS_KHAT] = ((double)n * kk + 5.0) / ((double)n + 10.0);
  }
}

__global__ __launch_bounds__(256) void psis_smooth_kernel(PsisArgs a) {
  const int rl = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, n = a.nt[rl];
  if (n <= 4 || i >= n) return;
  const double *st = a.state + (int64_t)rl * LOO_STATE;
  const double khat = st[LS_KHAT], sigma = st[LS_SIGMA];
  const double l1 = log1p(-((double)i + 0.5) / (double)n);
  const double q = (khat == 0.0) ? -sigma * l1 : sigma * expm1(-khat * l1) / khat;
  double v = log(st[LS_EXC] + q);
  if (v > 0.0) v = 0.0;       // truncation at the largest raw ratio
  a.smraw[(int64_t)rl * a.Mmax + i] = v;
}

__global__ __launch_bounds__(256) void psis_ties_kernel(PsisArgs a) {
  const int rl = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, n = a.nt[rl], S = a.S;
  if (n <= 4 || i >= n) return;
  const u64 *k = a.sorted + (int64_t)rl * S;
  const double vmin = a.state[(int64_t)rl * LOO_STATE + LS_VMIN];
  const double xi = psis_x(k, S, vmin, S - n + i);
  // the thread of a run's first position serves the whole run: linear in n whatever the runs' lengths
  if (i > 0 && psis_x(k, S, vmin, S - n + i - 1) == xi) return;
  const int64_t hi = psis_bound(k, S, vmin, S - n + i + 1, S, xi, true) - (S - n);
  const double *sm = a.smraw + (int64_t)rl * a.Mmax;
  double *out = a.smt + (int64_t)rl * a.Mmax;
  double v = sm[i];
  if (hi - i > 1) {
    double acc = 0.0;
    for (int64_t q = i; q < hi; ++q) acc += sm[q];
    v = acc / (double)(hi - i);
  }
  for (int64_t q = i; q < hi; ++q) out[q] = v;
}

// the unnormalised log-weight of an element of value v
static __device__ __forceinline__ double psis_lw(const PsisArgs &a, int rl, const double *st, int64_t n, double v) {
  const double vmin = st[LS_VMIN];
  const double x = vmin - v;
  if (n > 4 && x > st[LS_XC]) {
    const u64 *k = a.sorted + (int64_t)rl * a.S;
    int64_t p = psis_bound(k, a.S, vmin, a.S - n, a.S, x, false) - (a.S - n);
    if (p > n - 1) p = n - 1;
    return a.smt[(int64_t)rl * a.Mmax + p];
  }
  return x;
}

// workgroup (chunk c, row rl): part[.][0] = max lw, part[.][1] = max (lw + V) over the chunk
__global__ __launch_bounds__(256) void psis_max_kernel(PsisArgs a) {
  __shared__ double ws[4];
  const int rl = blockIdx.y, tid = threadIdx.x;
  const int64_t c = blockIdx.x, n = a.nt[rl];
  const double *st = a.state + (int64_t)rl * LOO_STATE;
  const double *row = a.V + (a.row0 + rl) * a.rs;
  double m0 = -INFINITY, m1 = -INFINITY;
  for (int j = 0; j < LOO_SUM / 256; ++j) {
    const int64_t i = c * LOO_SUM + (int64_t)j * 256 + tid;
    if (i < a.S) {
      const double v = row[i * a.es], lw = psis_lw(a, rl, st, n, v);
      m0 = fmax(m0, lw);
      m1 = fmax(m1, lw + v);
    }
  }
  m0 = wg_max_b<4>(m0, ws);
  m1 = wg_max_b<4>(m1, ws);
  if (tid == 0) {
    double *p = a.part + ((int64_t)rl * a.nchunk + c) * LOO_NSUM;
    p[0] = m0;
    p[1] = m1;
  }
}

__global__ __launch_bounds__(256) void psis_max_finish_kernel(PsisArgs a) {
  const int rl = blockIdx.x * 256 + threadIdx.x;
  if (rl >= a.rows) return;
  double m0 = -INFINITY, m1 = -INFINITY;
  for (int64_t c = 0; c < a.nchunk; ++c) {
    const double *p = a.part + ((int64_t)rl * a.nchunk + c) * LOO_NSUM;
    m0 = fmax(m0, p[0]);
    m1 = fmax(m1, p[1]);
  }
  a.state[(int64_t)rl * LOO_STATE + LS_MXW] = m0;
  a.state[(int64_t)rl * LOO_STATE + LS_MXE] = m1;
}

// chunk sums of exp(lw - mxw), exp(2 (lw - mxw)), exp(V - vmax), V, exp(lw + V - mxe)
__global__ __launch_bounds__(256) void psis_sum_kernel(PsisArgs a) {
  __shared__ double ws[4];
  const int rl = blockIdx.y, tid = threadIdx.x;
  const int64_t c = blockIdx.x, n = a.nt[rl];
  const double *st = a.state + (int64_t)rl * LOO_STATE;
  const double *row = a.V + (a.row0 + rl) * a.rs;
  const double mxw = st[LS_MXW], mxe = st[LS_MXE], vmax = st[LS_VMAX];
  double acc[LOO_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < LOO_SUM / 256; ++j) {
    const int64_t i = c * LOO_SUM + (int64_t)j * 256 + tid;
    if (i < a.S) {
      const double v = row[i * a.es], lw = psis_lw(a, rl, st, n, v);
      const double e = exp(lw - mxw);
      acc[0] += e;
      acc[1] += e * e;
      acc[2] += exp(v - vmax);
      acc[3] += v;
      acc[4] += exp(lw + v - mxe);
    }
  }
#pragma unroll
  for (int q = 0; q < LOO_NSUM; ++q) acc[q] = wg_sum_b<4>(acc[q], ws);
  if (tid == 0) {
    double *p = a.part + ((int64_t)rl * a.nchunk + c) * LOO_NSUM;
#pragma unroll
    for (int q = 0; q < LOO_NSUM; ++q) p[q] = acc[q];
  }
}

__global__ __launch_bounds__(256) void psis_sum_finish_kernel(PsisArgs a) {
  const int rl = blockIdx.x * 256 + threadIdx.x;
  if (rl >= a.rows) return;
  double acc[LOO_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t c = 0; c < a.nchunk; ++c) {
    const double *p = a.part + ((int64_t)rl * a.nchunk + c) * LOO_NSUM;
#pragma unroll
    for (int q = 0; q < LOO_NSUM; ++q) acc[q] += p[q];
  }
  double *st = a.state + (int64_t)rl * LOO_STATE;
  st[LS_A] = acc[0];
  st[LS_Q] = acc[1];
  st[LS_B] = acc[2];
  st[LS_MEANV] = acc[3] / (double)a.S;
  st[LS_E] = acc[4];
  st[LS_LSEW] = st[LS_MXW] + log(acc[0]);
}

// chunk sums of (V - mean)^2; the normalised log-weights in the input's order where asked for
__global__ __launch_bounds__(256) void psis_var_kernel(PsisArgs a) {
  __shared__ double ws[4];
  const int rl = blockIdx.y, tid = threadIdx.x;
  const int64_t c = blockIdx.x, n = a.nt[rl];
  const double *st = a.state + (int64_t)rl * LOO_STATE;
  const double *row = a.V + (a.row0 + rl) * a.rs;
  const double mean = st[LS_MEANV], lsew = st[LS_LSEW];
  const bool bad = a.nan[rl] != 0;
  double acc = 0.0;
  for (int j = 0; j < LOO_SUM / 256; ++j) {
    const int64_t i = c * LOO_SUM + (int64_t)j * 256 + tid;
    if (i < a.S) {
      const double v = row[i * a.es];
      acc += (v - mean) * (v - mean);
      if (a.logw) a.logw[(a.row0 + rl) * a.S + i] = bad ? loo_nan() : psis_lw(a, rl, st, n, v) - lsew;
    }
  }
  acc = wg_sum_b<4>(acc, ws);
  if (tid == 0) a.part[((int64_t)rl * a.nchunk + c) * LOO_NSUM] = acc;
}

__global__ __launch_bounds__(256) void psis_out_kernel(PsisArgs a) {
  const int rl = blockIdx.x * 256 + threadIdx.x;
  if (rl >= a.rows) return;
  double ssq = 0.0;
  for (int64_t c = 0; c < a.nchunk; ++c) ssq += a.part[((int64_t)rl * a.nchunk + c) * LOO_NSUM];
  const double *st = a.state + (int64_t)rl * LOO_STATE;
  double *o = a.out + (a.row0 + rl) * GPEMU_PSIS_NOUT;
  if (a.nan[rl]) {
    for (int q = 0; q < GPEMU_PSIS_NOUT; ++q) o[q] = loo_nan();
    return;
  }
  const double S = (double)a.S;
  const double elpd = (st[LS_MXE] + log(st[LS_E])) - st[LS_LSEW];
  const double lppd = (st[LS_VMAX] + log(st[LS_B])) - log(S);
  const double pw = ssq / (S - 1.0);   // 0 / 0 for S = 1
  o[GPEMU_PSIS_ELPD_LOO] = elpd;
  o[GPEMU_PSIS_LPPD] = lppd;
  o[GPEMU_PSIS_P_LOO] = lppd - elpd;
  o[GPEMU_PSIS_PARETO_K] = st[LS_KHAT];
  o[GPEMU_PSIS_N_TAIL] = (double)a.nt[rl];
  o[GPEMU_PSIS_ESS_W] = (st[LS_A] * st[LS_A]) / st[LS_Q];
  o[GPEMU_PSIS_P_WAIC] = pw;
  o[GPEMU_PSIS_ELPD_WAIC] = lppd - pw;
  o[GPEMU_PSIS_CUTOFF] = st[LS_XC];
}

static int psis_check(int64_t R, int64_t S, const double *r_eff) {
  GP_ARG(R > 0, "R must be positive");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  if (r_eff)
    for (int64_t r = 0; r < R; ++r) GP_ARG(std::isfinite(r_eff[r]) && r_eff[r] > 0.0, "every r_eff must be finite and > 0");
  return GPEMU_OK;
}

// the statistics of R rows, in batches of rows that fit workspace_bytes (0: half of the free memory); waits for st
static int psis_rows(const double *dV, int64_t R, int64_t S, int64_t rs, int64_t es, const double *r_eff, double *dout,
                     double *dlogw, int64_t workspace_bytes, hipStream_t st) {
  std::vector<int64_t> hM((size_t)R);
  int64_t Mmax = 1;
  for (int64_t r = 0; r < R; ++r) {
    const double re = r_eff ? r_eff[r] : 1.0;
    hM[(size_t)r] = (int64_t)std::ceil(std::min((double)S / 5.0, 3.0 * std::sqrt((double)S / re)));
    Mmax = std::max(Mmax, hM[(size_t)r]);
  }
  const int m_max = 30 + (int)std::floor(std::sqrt((double)Mmax));
  GP_ARG(m_max <= LOO_MAX_M, "the tail is too long for the fit's grid");
  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t nchunk = (S + LOO_SUM - 1) / LOO_SUM;
  const int64_t per_row = rank_row_bytes(S) + 16 * Mmax + 8 * LOO_NSUM * nchunk + 8 * LOO_STATE + 8 + 16 * LOO_MAX_M;
  int64_t rows_cap = sort_rows_cap(R, S, budget, per_row, 1);
  rows_cap = std::min<int64_t>(rows_cap, 65535);   // grid.y
  if (rows_cap < 1) {
    set_error("psis: out of memory: one row of %lld elements needs %lld bytes of sort, tail and partial-sum buffers; "
              "%lld bytes %s", (long long)S, (long long)per_row, (long long)budget, workspace_budget_name(workspace_bytes));
    return GPEMU_ERR_HIP;
  }
  DevScope sc(st);
  SortScratch sort;
  PsisArgs a;
  int64_t *dM = nullptr;
  GP_TRY(sort.alloc(sc, rows_cap, S));
  GP_TRY(sc.alloc(&dM, R));
  GP_TRY(sc.alloc(&a.state, rows_cap * LOO_STATE));
  GP_TRY(sc.alloc(&a.nt, rows_cap));
  GP_TRY(sc.alloc(&a.gb, rows_cap * LOO_MAX_M));
  GP_TRY(sc.alloc(&a.gL, rows_cap * LOO_MAX_M));
  GP_TRY(sc.alloc(&a.smraw, rows_cap * Mmax));
  GP_TRY(sc.alloc(&a.smt, rows_cap * Mmax));
  GP_TRY(sc.alloc(&a.part, rows_cap * nchunk * LOO_NSUM));
  GP_TRY(upload(dM, hM.data(), R, st));
  a.V = dV; a.rs = rs; a.es = es; a.S = S;
  a.sorted = sort.ka; a.nan = sort.nan; a.M = dM; a.Mmax = Mmax; a.nchunk = nchunk;
  a.log_tiny = std::log(DBL_MIN);
  a.out = dout; a.logw = dlogw;
  std::vector<long long> hn((size_t)rows_cap);
  for (int64_t row0 = 0; row0 < R; row0 += rows_cap) {
    const int64_t rows = std::min(rows_cap, R - row0);
    a.row0 = row0;
    a.rows = (int)rows;
    loo_path_count(GPEMU_LOO_PATH_ROW_BATCH);
    GP_TRY(sort_rows(dV, rs, es, S, row0, rows, sort, [] { loo_path_count(GPEMU_LOO_PATH_SORT_PASS); }, st));
    const dim3 per_row_grid((unsigned)((rows + 255) / 256)), tail_grid((unsigned)((Mmax + 255) / 256), (unsigned)rows);
    const dim3 chunk_grid((unsigned)nchunk, (unsigned)rows);
    hipLaunchKernelGGL(psis_tail_kernel, per_row_grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(psis_gpd_k_kernel, dim3((unsigned)m_max, (unsigned)rows), dim3(256), 0, st, a);
    hipLaunchKernelGGL(psis_gpd_fit_kernel, dim3((unsigned)rows), dim3(256), 0, st, a);
    hipLaunchKernelGGL(psis_smooth_kernel, tail_grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(psis_ties_kernel, tail_grid, dim3(256), 0, st, a);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(psis_max_kernel, chunk_grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(psis_max_finish_kernel, per_row_grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(psis_sum_kernel, chunk_grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(psis_sum_finish_kernel, per_row_grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(psis_var_kernel, chunk_grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(psis_out_kernel, per_row_grid, dim3(256), 0, st, a);
    GP_HIP(hipGetLastError());
    GP_TRY(sc.download(hn.data(), a.nt, rows));
    GP_HIP(hipStreamSynchronize(st));
    for (int64_t r = 0; r < rows; ++r)
      loo_path_count(hn[(size_t)r] > 4 ? GPEMU_LOO_PATH_ROW_SMOOTHED : GPEMU_LOO_PATH_ROW_RAW);
  }
  GP_HIP(hipStreamSynchronize(st));   // hM is read by the copy above
  return GPEMU_OK;
}

// ---- weighted moments of the parameters ----------------------------------------------------------------------------
constexpr int WM_MAX_D = 16;
struct WmArgs {
  RowsView X;
  int64_t S, nchunk, ldw;
  const double *logw;          // [R][ldw]
  const double *mean;          // [R][d]: the second pass; null: the first
  double *part;                // [R][nchunk][WM_MAX_D + 1]
};

// workgroup (chunk c, weight row r): the chunk's sums of w x_j (or w (x_j - mean_j)^2) and of w = exp(logw)
__global__ __launch_bounds__(256) void wm_partial_kernel(WmArgs a) {
  __shared__ double ws[4];
  const int tid = threadIdx.x, d = a.X.d;
  const int64_t c = blockIdx.x, r = blockIdx.y;
  double acc[WM_MAX_D + 1];
  double mu[WM_MAX_D];
#pragma unroll
  for (int j = 0; j <= WM_MAX_D; ++j) acc[j] = 0.0;
#pragma unroll
  for (int j = 0; j < WM_MAX_D; ++j) mu[j] = (a.mean && j < d) ? a.mean[r * d + j] : 0.0;
  for (int q = 0; q < LOO_SUM / 256; ++q) {
    const int64_t i = c * LOO_SUM + (int64_t)q * 256 + tid;
    if (i < a.S) {
      const double w = exp(a.logw[r * a.ldw + i]);
      const double *x = a.X.row(i);
      acc[WM_MAX_D] += w;
#pragma unroll
      for (int j = 0; j < WM_MAX_D; ++j)
        if (j < d) {
          const double t = x[j] - mu[j];
          acc[j] += a.mean ? w * (t * t) : w * t;
        }
    }
  }
  double *p = a.part + (r * a.nchunk + c) * (WM_MAX_D + 1);
#pragma unroll
  for (int j = 0; j <= WM_MAX_D; ++j) {
    if (j < d || j == WM_MAX_D) {
      const double v = wg_sum_b<4>(acc[j], ws);
      if (tid == 0) p[j] = v;
    }
  }
}

// out[r][j] = (the chunk sums of column j, in chunk order) / (those of the weights)
__global__ __launch_bounds__(256) void wm_finish_kernel(const double *__restrict__ part, int64_t R, int d, int64_t nchunk,
                                                        double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= R * d) return;
  const int64_t r = i / d;
  const int j = (int)(i % d);
  double s = 0.0, w = 0.0;
  for (int64_t c = 0; c < nchunk; ++c) {
    const double *p = part + (r * nchunk + c) * (WM_MAX_D + 1);
    s += p[j];
    w += p[WM_MAX_D];
  }
  out[i] = s / w;
}

// out[g ldo + s] = the sum of rows idx[start[g] .. start[g + 1]) of T at s, added in the given order
__global__ __launch_bounds__(256) void loo_group_rows_kernel(const double *__restrict__ T, int64_t ldt, int64_t S,
                                                             const int64_t *__restrict__ start,
                                                             const int64_t *__restrict__ idx, double *__restrict__ out,
                                                             int64_t ldo) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
  if (s >= S) return;
  double acc = T[idx[start[g]] * ldt + s];
  for (int64_t q = start[g] + 1; q < start[g + 1]; ++q) acc += T[idx[q] * ldt + s];
  out[g * ldo + s] = acc;
}

// what the terms calls decline, before anything is allocated or launched
static int pointwise_check(const gpemu_model *m, int chain) {
  if (!m->lik_ready) { set_error("gpemu_likelihood_setup has not been called"); return GPEMU_ERR_STATE; }
  if (m->n_src > 0) {
    set_error("loglik_pointwise: correlated sources (n_src = %d) span the observable blocks: the likelihood does not "
              "factorise over them", m->n_src);
    return GPEMU_ERR_UNSUPPORTED;
  }
  GP_ARG(chain >= 0 && chain < m->lik_chains, "chain must be in [0, the data vectors of the likelihood setup)");
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_loo_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_LOO, out, n); }

int gpemu_model_observable_blocks(const gpemu_model *m, int64_t *n_blocks) {
  GP_ARG(m && n_blocks, "null pointer");
  if (!m->lik_ready) { set_error("gpemu_likelihood_setup has not been called"); return GPEMU_ERR_STATE; }
  *n_blocks = m->nblk;
  return GPEMU_OK;
}

int gpemu_loglik_pointwise_dev(gpemu_model *m, int chain, const double *dX, int64_t n_blocks, int64_t block_rows,
                               int64_t block_stride_rows, double *dT, int64_t ldt, void *stream) {
  GP_ARG(m && dX && dT, "null pointer");
  GP_TRY(pointwise_check(m, chain));
  const RowsView X{dX, n_blocks, block_rows, block_stride_rows * m->d, (int)m->d};
  GP_TRY(rows_check(X));
  GP_ARG(n_blocks <= INT64_MAX / block_rows, "n_blocks * block_rows overflows");
  const int64_t S = n_blocks * block_rows, k = m->k, d = m->d, nblk = m->nblk;
  GP_ARG(ldt >= S, "ldt must be at least the number of rows");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;

  DevScope sc(st);
  double *Mpc = nullptr, *Vpc = nullptr, *stage = nullptr;
  GP_TRY(sc.alloc(&Mpc, LOO_CHUNK * k));
  GP_TRY(sc.alloc(&Vpc, LOO_CHUNK * k));
  if (!X.dense()) GP_TRY(sc.alloc(&stage, LOO_CHUNK * d));
  TermArgs a;
  a.X = X;
  a.mean = Mpc; a.var = Vpc;
  a.G = m->G;
  a.g0 = m->g0 + (int64_t)chain * nblk * k;
  a.scal = m->scal + (int64_t)chain * 2 * nblk;
  a.k = (int)k; a.nblk = (int)nblk;
  a.T = dT; a.ldt = ldt;
  for (int64_t r0 = 0; r0 < S; r0 += LOO_CHUNK) {
    const int64_t nb = std::min(LOO_CHUNK, S - r0);
    const double *src = stage;
    if (X.dense())
      src = dX + r0 * d;
    else if (r0 / block_rows == (r0 + nb - 1) / block_rows)   // the chunk lies within one block
      src = X.row(r0);
    else
      GP_TRY(gather_rows(X, r0, nb, stage, st));
    loo_path_count(GPEMU_LOO_PATH_CHUNK);
    GP_TRY(gpemu_gp_predict_dev(m, nb, src, Mpc, Vpc, st));
    a.r0 = r0; a.nb = nb;
    GP_TRY(launch_loo_terms(a, st));
  }
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_loglik_pointwise(gpemu_model *m, int chain, int64_t B, const double *X, double *T) {
  GP_ARG(m && X && T, "null pointer");
  GP_ARG(B > 0, "B must be positive");
  GP_TRY(pointwise_check(m, chain));   // declined calls allocate and copy nothing
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  DevScope sc(st);
  double *dX = nullptr, *dT = nullptr;
  GP_TRY(sc.alloc(&dX, B * m->d));
  GP_TRY(sc.alloc(&dT, B * m->nblk));
  GP_TRY(upload(dX, X, B * m->d, st));
  GP_TRY(gpemu_loglik_pointwise_dev(m, chain, dX, 1, B, B, dT, B, st));
  GP_TRY(sc.download(T, dT, B * m->nblk));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_psis_dev(int device, int64_t R, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                   const double *r_eff, double *dout, double *dlogw, int64_t workspace_bytes, void *stream) {
  GP_ARG(dV && dout, "null pointer");
  GP_TRY(psis_check(R, S, r_eff));
  GP_ARG(row_stride > 0 && elem_stride > 0, "strides must be positive");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_TRY(device_ready(device));
  return psis_rows(dV, R, S, row_stride, elem_stride, r_eff, dout, dlogw, workspace_bytes, (hipStream_t)stream);
}

int gpemu_psis(int device, int64_t R, int64_t S, const double *V, const double *r_eff, int64_t workspace_bytes, double *out,
               double *logw) {
  GP_ARG(V && out, "null pointer");
  GP_TRY(psis_check(R, S, r_eff));
  GP_ARG(R <= INT64_MAX / 8 / S, "R * S overflows");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  DevScope sc(st);
  double *dV = nullptr, *dout = nullptr, *dlw = nullptr;
  GP_TRY(sc.alloc(&dV, R * S));
  GP_TRY(sc.alloc(&dout, R * GPEMU_PSIS_NOUT));
  if (logw) GP_TRY(sc.alloc(&dlw, R * S));
  GP_TRY(upload(dV, V, R * S, st));
  GP_TRY(psis_rows(dV, R, S, S, 1, r_eff, dout, dlw, workspace_bytes, st));
  GP_TRY(sc.download(out, dout, R * GPEMU_PSIS_NOUT));
  if (logw) GP_TRY(sc.download(logw, dlw, R * S));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_weighted_moments_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows,
                               int64_t block_stride_rows, int d, int64_t R, const double *dlogw, int64_t ldw,
                               double *dmean, double *dvar, void *stream) {
  GP_ARG(dX && dlogw && dmean && dvar, "null pointer");
  GP_ARG(d >= 1 && d <= WM_MAX_D, "d must be in [1, 16]");
  const RowsView X{dX, n_blocks, block_rows, block_stride_rows * d, d};
  GP_TRY(rows_check(X));
  GP_ARG(n_blocks <= ((1ll << 31) - 1) / block_rows, "S = n_blocks * block_rows must be below 2^31");
  const int64_t S = n_blocks * block_rows;
  GP_ARG(R >= 1 && R <= 65535, "R must be in [1, 65535]");
  GP_ARG(ldw >= S, "ldw must be at least the number of rows");
  GP_TRY(device_ready(device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t nchunk = (S + LOO_SUM - 1) / LOO_SUM;
  DevScope sc(st);
  WmArgs a;
  GP_TRY(sc.alloc(&a.part, R * nchunk * (WM_MAX_D + 1)));
  a.X = X; a.S = S; a.nchunk = nchunk; a.ldw = ldw; a.logw = dlogw;
  const dim3 grid((unsigned)nchunk, (unsigned)R), fin((unsigned)((R * d + 255) / 256));
  a.mean = nullptr;
  hipLaunchKernelGGL(wm_partial_kernel, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(wm_finish_kernel, fin, dim3(256), 0, st, a.part, R, d, nchunk, dmean);
  a.mean = dmean;
  hipLaunchKernelGGL(wm_partial_kernel, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(wm_finish_kernel, fin, dim3(256), 0, st, a.part, R, d, nchunk, dvar);
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_loo_group_rows_dev(int device, int64_t R, int64_t S, const double *dT, int64_t ldt, int64_t n_groups,
                             const int64_t *group_start, const int64_t *rows, double *dout, int64_t ldo, void *stream) {
  GP_ARG(dT && dout && group_start && rows, "null pointer");
  GP_ARG(R >= 1 && S >= 1 && ldt >= S && ldo >= S, "R, S must be positive and the leading dimensions at least S");
  GP_ARG(n_groups >= 1 && n_groups <= 65535, "n_groups must be in [1, 65535]");
  GP_ARG(group_start[0] == 0, "group_start must begin at 0");
  for (int64_t g = 0; g < n_groups; ++g) GP_ARG(group_start[g + 1] > group_start[g], "every group must name a row");
  for (int64_t q = 0; q < group_start[n_groups]; ++q) GP_ARG(rows[q] >= 0 && rows[q] < R, "every row must be in [0, R)");
  GP_TRY(device_ready(device));
  hipStream_t st = (hipStream_t)stream;
  DevScope sc(st);
  int64_t *dstart = nullptr, *didx = nullptr;
  GP_TRY(sc.alloc(&dstart, n_groups + 1));
  GP_TRY(sc.alloc(&didx, group_start[n_groups]));
  GP_TRY(upload(dstart, group_start, n_groups + 1, st));
  GP_TRY(upload(didx, rows, group_start[n_groups], st));
  hipLaunchKernelGGL(loo_group_rows_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)n_groups), dim3(256), 0, st, dT, ldt,
                     S, dstart, didx, dout, ldo);
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

}  // extern "C"
