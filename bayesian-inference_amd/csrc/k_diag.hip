// Exact average ranks of many rows at once (gpemu_rank*) and the transformed split chains behind rank-normalised
// split-Rhat and bulk / tail ESS (gpemu_diag_*; Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021).
//
// Ranks: the key-only LSD radix sort of k_rows.hip (order-preserving 64-bit keys, eight stable 8-bit passes), then two
// binary searches per element.
// rk_lookup_kernel finds, for every element, the number of sorted keys below it (lo) and not above it (hi): the ranks
// lo + 1 .. hi are tied, their average is (lo + hi + 1) / 2, exact in a double.  The sorted key array of a row is unique
// and every counter is an integer: the ranks do not depend on the grid, on the batch of rows or on the run.
//
// Diagnostics: the handle gathers the split chains into Y[N][2 nw d] (diag_split_kernel), rank-normalises Y in place
// (the sort reads parameter dd as the row with row_stride 1, elem_stride d; the lookup writes normcdfinv of the rank's
// probability over the value it read), and runs k_acf.hip's kernels on Y with ld = S: per-series means (acf_sum_kernel,
// acf_mean_kernel), centred squares (diag_ss_kernel, the same chunks), lag products (acf_lag_kernel, acf_reduce_kernel).
// diag_chain_reduce_kernel is the fixed-order sum over the 2 nw chains of one parameter (a lane-strided sum in chain
// order, then tree B of wg_dev.h).  A median or quantile of the pooled unsplit segment comes from gpemu_select_dev on a
// dense copy of the segment, which uses Y's buffer before Y is written.
#include <algorithm>

#include "internal.h"
#include "rows_dev.h"
#include "sampler_internal.h"
#include "wg_dev.h"

namespace gpemu {

constexpr int DIAG_RANGE_CHUNKS = 128;

static inline void diag_path_count(int path) { count_path(PATHS_DIAG, path); }   // enum gpemu_diag_path

// out[(row0 + rl) out_rs + i out_es] = the average rank of element i (Z: normcdfinv((rank - 3/8) / (S + 1/4))), NaN for
// a row with a NaN.  out may be V itself: a thread writes only where it has read
template <bool Z>
__global__ __launch_bounds__(256) void rk_lookup_kernel(const double *V, int64_t row_stride, int64_t elem_stride,
                                                        int64_t S, int64_t row0, int64_t nblk,
                                                        const u64 *__restrict__ sorted, const int *__restrict__ nan,
                                                        double *out, int64_t out_rs, int64_t out_es) {
  const int64_t rl = blockIdx.x / nblk, i = (blockIdx.x % nblk) * 256 + threadIdx.x;
  if (i >= S) return;
  const u64 key = rk_key(V[(row0 + rl) * row_stride + i * elem_stride]);
  const u64 *k = sorted + rl * S;
  int64_t a = 0, b = S;            // lo: the first index with k[idx] >= key
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if (k[m] < key) a = m + 1; else b = m;
  }
  const int64_t lo = a;
  b = S;                           // hi: the first index with k[idx] > key (from lo on)
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if (k[m] <= key) a = m + 1; else b = m;
  }
  double r = (double)(lo + a + 1) * 0.5;
  if (Z) r = normcdfinv((r - 0.375) / ((double)S + 0.25));
  if (nan[rl]) r = __longlong_as_double(0x7ff8000000000000ll);
  out[(row0 + rl) * out_rs + i * out_es] = r;
}

// ranks (or their normal scores) of R rows, in batches of rows that fit workspace_bytes (0: half of the free memory);
// works on st and waits for it.  The caller has checked the arguments.
static int rank_rows(const double *dV, int64_t R, int64_t S, int64_t row_stride, int64_t elem_stride, double *dout,
                     int64_t out_rs, int64_t out_es, bool z, int64_t workspace_bytes, hipStream_t st) {
  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t nblk = (S + 255) / 256, per_row = rank_row_bytes(S), rows_cap = sort_rows_cap(R, S, budget, per_row);
  if (rows_cap < 1) {
    set_error("rank: out of memory: one row of %lld elements needs %lld bytes of sort buffers; %lld bytes %s", (long long)S,
              (long long)per_row, (long long)budget, workspace_budget_name(workspace_bytes));
    return GPEMU_ERR_HIP;
  }
  DevScope sc(st);
  SortScratch sort;
  GP_TRY(sort.alloc(sc, rows_cap, S));
  for (int64_t row0 = 0; row0 < R; row0 += rows_cap) {
    const int64_t rows = std::min(rows_cap, R - row0);
    diag_path_count(GPEMU_DIAG_PATH_ROW_BATCH);
    GP_TRY(sort_rows(dV, row_stride, elem_stride, S, row0, rows, sort, [] { diag_path_count(GPEMU_DIAG_PATH_SORT_PASS); },
                     st));
    diag_path_count(GPEMU_DIAG_PATH_RANK_LOOKUP);
    if (z)
      hipLaunchKernelGGL(rk_lookup_kernel<true>, dim3((unsigned)(rows * nblk)), dim3(256), 0, st, dV, row_stride,
                         elem_stride, S, row0, nblk, (const u64 *)sort.ka, (const int *)sort.nan, dout, out_rs, out_es);
    else
      hipLaunchKernelGGL(rk_lookup_kernel<false>, dim3((unsigned)(rows * nblk)), dim3(256), 0, st, dV, row_stride,
                         elem_stride, S, row0, nblk, (const u64 *)sort.ka, (const int *)sort.nan, dout, out_rs, out_es);
    GP_HIP(hipGetLastError());
  }
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

static int rank_check(int64_t R, int64_t S) {
  GP_ARG(R > 0, "R must be positive");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  return GPEMU_OK;
}

// ---- the transformed split chains ----------------------------------------------------------------------------------
// Y[t][(h nw + w) d + dd] = op(x[h ? n - N + t : t][w][dd]): identity, |x - par[dd]| or 1[x <= par[dd]]
__global__ __launch_bounds__(256) void diag_split_kernel(const double *__restrict__ src, int64_t step_stride, int64_t n,
                                                         int64_t N, int64_t nw, int d, int op,
                                                         const double *__restrict__ par, double *__restrict__ Y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t wd = nw * d;
  if (i >= N * 2 * wd) return;
  const int64_t t = i / (2 * wd), rem = i % (2 * wd), h = rem / wd, c = rem % wd;
  double v = src[(h ? n - N + t : t) * step_stride + c];
  if (op == 1) v = fabs(v - par[c % d]);
  if (op == 2) v = (v <= par[c % d]) ? 1.0 : 0.0;
  Y[i] = v;
}

// part[c][s] = sum over the steps of chunk c of (y - mean[s])^2: acf_sum_kernel's chunks and order
__global__ __launch_bounds__(256) void diag_ss_kernel(const double *__restrict__ Y, const double *__restrict__ mean,
                                                      int64_t n_t, int64_t S, int64_t tchunk, double *__restrict__ part) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const int64_t t0 = (int64_t)blockIdx.z * tchunk, t1 = std::min<int64_t>(t0 + tchunk, n_t);
  const double mu = mean[s];
  double a0 = 0.0, a1 = 0.0;
  int64_t t = t0;
  for (; t + 2 <= t1; t += 2) {
    const double u = Y[t * S + s] - mu, v = Y[(t + 1) * S + s] - mu;
    a0 = fma(u, u, a0);
    a1 = fma(v, v, a1);
  }
  if (t < t1) {
    const double u = Y[t * S + s] - mu;
    a0 = fma(u, u, a0);
  }
  part[(int64_t)blockIdx.z * S + s] = a0 + a1;
}

// out[l d + dd] = scale * sum over the K chains k of f(in[l S + k d + dd]), f(v) = v or, with a centre, (v - centre[dd])^2:
// the lanes add their chains in order, then tree B (wg_dev.h); workgroup (l, dd)
__global__ __launch_bounds__(256) void diag_chain_reduce_kernel(const double *__restrict__ in, int64_t S, int d, int64_t K,
                                                                const double *__restrict__ centre, double scale,
                                                                double *__restrict__ out) {
  __shared__ double ws[4];
  const int64_t l = blockIdx.x;
  const int dd = blockIdx.y;
  const double c = centre ? centre[dd] : 0.0;
  double a = 0.0;
  for (int64_t k = threadIdx.x; k < K; k += 256) {
    const double v = in[l * S + k * d + dd] - c;
    a += centre ? v * v : v;
  }
  a = wg_sum_b<4>(a, ws);
  if (threadIdx.x == 0) out[l * d + dd] = a * scale;
}

// omin / omax[c d + dd] = min / max of imin / imax[e d + dd] over the elements e of chunk c (tree A); workgroup (dd, c)
__global__ __launch_bounds__(256) void diag_range_kernel(const double *__restrict__ imin, const double *__restrict__ imax,
                                                         int64_t count, int d, double *__restrict__ omin,
                                                         double *__restrict__ omax) {
  __shared__ double red[256];
  const int tid = threadIdx.x, dd = blockIdx.x;
  const int64_t per = (count + gridDim.y - 1) / gridDim.y, e0 = (int64_t)blockIdx.y * per, e1 = std::min(e0 + per, count);
  double a = INFINITY, b = -INFINITY;
  for (int64_t e = e0 + tid; e < e1; e += 256) {
    a = fmin(a, imin[e * d + dd]);
    b = fmax(b, imax[e * d + dd]);
  }
  a = wg_min_a<256>(a, red);
  b = wg_max_a<256>(b, red);
  if (tid == 0) {
    omin[(int64_t)blockIdx.y * d + dd] = a;
    omax[(int64_t)blockIdx.y * d + dd] = b;
  }
}

}  // namespace gpemu

using namespace gpemu;

struct gpemu_diag {
  int device = 0;
  hipStream_t stream = nullptr;
  const double *src = nullptr;     // walker w0 of the first step of the segment
  double *owned = nullptr;         // the device copy of a host chain (gpemu_diag_create)
  gpemu_sampler *sampler = nullptr;  // the sampler whose chain is borrowed, and the epoch it was borrowed at
  uint64_t epoch = 0;
  int64_t n = 0, N = 0, step_stride = 0, nw = 0, K = 0, S = 0, workspace_bytes = 0;
  int d = 0;
  double *Y = nullptr;             // [n nw d]: Y[N][S], or the dense segment
  double *mean = nullptr, *var = nullptr, *acf0 = nullptr;   // [S] per-series mean, ddof-1 variance, lag-0 products
  double *small = nullptr;         // [8 d + 2 DIAG_RANGE_CHUNKS d] parameters, moments, ranges
  double *part = nullptr, *acf = nullptr;
  size_t part_bytes = 0, acf_bytes = 0;
  int kind = -1;                   // the transform Y holds; -1: none
  bool acov_started = false;
  bool pooled_ready = false;
  std::vector<double> pooled;      // mean | sd | median | min | max, [d] each
};

namespace gpemu {

static int diag_fresh(const gpemu_diag *h) {
  if (h->sampler && h->sampler->chain_epoch != h->epoch) {
    set_error("gpemu_diag: the sampler's chain has been run, reserved, reset or restored since it was borrowed");
    return GPEMU_ERR_STATE;
  }
  return GPEMU_OK;
}

static int diag_chunks(const gpemu_diag *h, int64_t *tchunk) {
  const int nchunk = (int)std::min<int64_t>(ACF_TCHUNKS, (h->N + ACF_LPT - 1) / ACF_LPT);
  *tchunk = round_up((h->N + nchunk - 1) / nchunk, ACF_LPT);
  return nchunk;
}

static int diag_new(gpemu_diag **out, int device, hipStream_t st, const double *src, double *owned, int64_t n,
                    int64_t step_stride, int64_t nw, int d, int64_t workspace_bytes) {
  gpemu_diag *h = new gpemu_diag;
  h->device = device; h->stream = st; h->src = src; h->owned = owned;
  h->n = n; h->N = n / 2; h->step_stride = step_stride; h->nw = nw; h->K = 2 * nw; h->S = 2 * nw * d; h->d = d;
  h->workspace_bytes = workspace_bytes;
  int rc = dev_alloc(&h->Y, n * nw * d);
  if (rc == GPEMU_OK) rc = dev_alloc(&h->mean, h->S);
  if (rc == GPEMU_OK) rc = dev_alloc(&h->var, h->S);
  if (rc == GPEMU_OK) rc = dev_alloc(&h->acf0, h->S);
  if (rc == GPEMU_OK) rc = dev_alloc(&h->small, (int64_t)(8 + 2 * DIAG_RANGE_CHUNKS) * d);
  if (rc != GPEMU_OK) {
    gpemu_diag_destroy(h);
    return rc;
  }
  *out = h;
  return GPEMU_OK;
}

// the segment as rows in blocks (a step is a block) within the handle's own limits
static int diag_view_check(int64_t n, int64_t step_stride, int64_t nw, int d) {
  GP_TRY(rows_check(RowsView{nullptr, n, nw, step_stride, d}));
  GP_ARG(n >= 8, "n must be at least 8 (N = n / 2 >= 4)");
  GP_ARG(d <= 65535, "d must be in [1, 65535]");
  GP_ARG(n <= ((1ll << 31) - 1) / nw, "n * nw must be below 2^31");
  return GPEMU_OK;
}

// the dense unsplit segment into Y's buffer (Y is no transform after this)
static int diag_dense(gpemu_diag *h) {
  h->kind = -1;
  return gather_rows(RowsView{h->src, h->n, h->nw, h->step_stride, h->d}, 0, h->n * h->nw, h->Y, h->stream);
}

// order statistics ranks[0 .. nr) of every parameter of the pooled unsplit segment -> host out[dd nr + i]
static int diag_select(gpemu_diag *h, int nr, const int64_t *ranks, double *out) {
  GP_TRY(diag_dense(h));
  DevScope sc(h->stream);
  double *dq = nullptr;
  GP_TRY(sc.alloc(&dq, (int64_t)h->d * nr));
  GP_TRY(gpemu_select_dev(h->device, h->d, h->n * h->nw, h->Y, 1, h->d, nr, ranks, dq, (void *)h->stream));
  GP_TRY(sc.download(out, dq, (int64_t)h->d * nr));
  GP_HIP(hipStreamSynchronize(h->stream));
  return GPEMU_OK;
}

static int diag_ensure_pooled(gpemu_diag *h) {
  if (h->pooled_ready) return GPEMU_OK;
  const int d = h->d;
  const int64_t T = h->n * h->nw;
  int64_t ranks[4] = {0, (T - 1) / 2, T / 2, T - 1};
  int nr = 0;
  int where[4];
  for (int i = 0; i < 4; ++i) {   // distinct ranks only
    if (nr == 0 || ranks[nr - 1] != ranks[i]) ranks[nr++] = ranks[i];
    where[i] = nr - 1;
  }
  std::vector<double> q((size_t)d * 4);
  GP_TRY(diag_select(h, nr, ranks, q.data()));   // leaves the dense segment in Y
  std::vector<double> mom((size_t)2 * d);
  GP_TRY(moments_to_host(h->Y, T, d, mom.data(), mom.data() + d, h->stream));
  h->pooled.assign((size_t)5 * d, 0.0);
  for (int dd = 0; dd < d; ++dd) {
    const double *qd = q.data() + (size_t)dd * nr;
    h->pooled[dd] = mom[dd];
    h->pooled[d + dd] = std::sqrt(mom[d + dd] * ((double)T / (double)(T - 1)));
    h->pooled[2 * d + dd] = (qd[where[1]] + qd[where[2]]) / 2.0;   // np.median: the mean of the middle pair
    h->pooled[3 * d + dd] = qd[where[0]];
    h->pooled[4 * d + dd] = qd[where[3]];
  }
  h->pooled_ready = true;
  return GPEMU_OK;
}

// np.quantile(pooled unsplit segment, prob, method='linear') per parameter, as gpemu.select.quantile: numpy's virtual
// index and _lerp, each product and sum rounded on its own
static int diag_quantile(gpemu_diag *h, double prob, double *q_out) {
#pragma clang fp contract(off)
  const int64_t T = h->n * h->nw;
  const double v = (double)(T - 1) * prob;
  const int64_t lo = (int64_t)std::floor(v), hi = std::min<int64_t>(lo + 1, T - 1);
  const double t = v - (double)lo;
  int64_t ranks[2] = {lo, hi};
  const int nr = hi > lo ? 2 : 1;
  std::vector<double> q((size_t)h->d * 2);
  GP_TRY(diag_select(h, nr, ranks, q.data()));
  for (int dd = 0; dd < h->d; ++dd) {
    const double a = q[(size_t)dd * nr], b = q[(size_t)dd * nr + (nr - 1)];
    const double diff = b - a;
    double r;
    if (t >= 0.5) {
      const double u = 1.0 - t, p = diff * u;
      r = b - p;
    } else {
      const double p = diff * t;
      r = a + p;
    }
    q_out[dd] = t == 0.0 ? a : r;
  }
  return GPEMU_OK;
}

}  // namespace gpemu

extern "C" {

int gpemu_diag_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_DIAG, out, n); }

int gpemu_rank_dev(int device, int64_t R, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                   double *dranks, int64_t workspace_bytes, void *stream) {
  GP_ARG(dV && dranks, "null pointer");
  GP_TRY(rank_check(R, S));
  GP_ARG(row_stride > 0 && elem_stride > 0, "strides must be positive");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_TRY(device_ready(device));
  return rank_rows(dV, R, S, row_stride, elem_stride, dranks, S, 1, false, workspace_bytes, (hipStream_t)stream);
}

int gpemu_rank(int device, int64_t R, int64_t S, const double *V, double *ranks_out) {
  GP_ARG(V && ranks_out, "null pointer");
  GP_TRY(rank_check(R, S));
  GP_ARG(R <= INT64_MAX / 8 / S, "R * S overflows");
  return with_host_rows(device, R, S, V, S, ranks_out, [&](const double *dV, double *dr, hipStream_t st) {
    return rank_rows(dV, R, S, S, 1, dr, S, 1, false, 0, st);
  });
}

int gpemu_diag_create(gpemu_diag **out, int device, const double *chain, int64_t n, int64_t W, int d) {
  GP_ARG(out && chain, "null pointer");
  GP_ARG(W <= INT64_MAX / 8 / std::max(d, 1), "W * d overflows");
  GP_TRY(diag_view_check(n, W * d, W, d));
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  double *dchain = nullptr;
  {
    DevScope sc(st);
    GP_TRY(sc.alloc(&dchain, n * W * d));
    GP_TRY(upload(dchain, chain, n * W * d, st));
    GP_HIP(hipStreamSynchronize(st));
    sc.release(dchain);
  }
  return diag_new(out, device, st, dchain, dchain, n, W * d, W, d, 0);   // the handle owns the copy, also where it fails
}

int gpemu_diag_create_dev(gpemu_diag **out, int device, const double *dchain, int64_t n, int64_t step_stride, int64_t w0,
                          int64_t nw, int d, int64_t workspace_bytes, void *stream) {
  GP_ARG(out && dchain, "null pointer");
  GP_TRY(diag_view_check(n, step_stride, nw, d));
  GP_ARG(w0 >= 0, "w0 must be >= 0");
  GP_ARG(step_stride >= (w0 + nw) * d, "step_stride must hold walkers [0, w0 + nw)");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_TRY(device_ready(device));
  return diag_new(out, device, (hipStream_t)stream, dchain + w0 * d, nullptr, n, step_stride, nw, d, workspace_bytes);
}

int gpemu_sampler_diag_create(gpemu_diag **out, gpemu_sampler *s, int64_t first, int64_t n, int64_t thin, int64_t w0,
                              int64_t nw) {
  GP_ARG(out && s, "null pointer");
  GP_ARG(thin >= 1, "thin must be positive");
  GP_ARG(w0 >= 0 && nw >= 1 && w0 + nw <= s->W, "walker range");
  GP_TRY(diag_view_check(n, thin * s->W * s->d, nw, (int)s->d));
  GP_ARG(first >= 0 && first < s->chain_len && (n - 1) <= (s->chain_len - 1 - first) / thin, "chain range");
  GP_HIP(hipSetDevice(s->device));
  GP_TRY(diag_new(out, s->device, s->stream, s->chain + first * s->W * s->d + w0 * s->d, nullptr, n, thin * s->W * s->d, nw,
                  (int)s->d, 0));
  (*out)->sampler = s;
  (*out)->epoch = s->chain_epoch;
  return GPEMU_OK;
}

void gpemu_diag_destroy(gpemu_diag *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  dev_free(h->Y); dev_free(h->mean); dev_free(h->var); dev_free(h->acf0); dev_free(h->small);
  dev_free(h->part); dev_free(h->acf); dev_free(h->owned);
  delete h;
}

int gpemu_diag_pooled(gpemu_diag *h, double *mean, double *sd_ddof1, double *median, double *min, double *max) {
  GP_ARG(h, "null handle");
  GP_TRY(diag_fresh(h));
  GP_HIP(hipSetDevice(h->device));
  GP_TRY(diag_ensure_pooled(h));
  double *dst[5] = {mean, sd_ddof1, median, min, max};
  for (int i = 0; i < 5; ++i)
    if (dst[i]) std::copy(h->pooled.begin() + (size_t)i * h->d, h->pooled.begin() + (size_t)(i + 1) * h->d, dst[i]);
  return GPEMU_OK;
}

int gpemu_diag_transform(gpemu_diag *h, int kind, double prob, double *grand_mean, double *mean_var,
                         double *var_of_means) {
  GP_ARG(h && grand_mean && mean_var && var_of_means, "null pointer");
  GP_ARG(kind >= GPEMU_DIAG_IDENTITY && kind <= GPEMU_DIAG_INDICATOR_LE, "unknown kind");
  GP_ARG(kind != GPEMU_DIAG_INDICATOR_LE || (prob >= 0.0 && prob <= 1.0), "prob must be in [0, 1]");
  GP_TRY(diag_fresh(h));
  GP_HIP(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const int d = h->d;
  const int64_t N = h->N, S = h->S, K = h->K;
  h->kind = -1;
  h->acov_started = false;
  // the parameter of the fold / the indicator: [d] at small
  double *dpar = h->small;
  std::vector<double> par((size_t)d);
  int op = 0;
  if (kind == GPEMU_DIAG_FOLDED_RANK_Z) {
    GP_TRY(diag_ensure_pooled(h));
    std::copy(h->pooled.begin() + 2 * (size_t)d, h->pooled.begin() + 3 * (size_t)d, par.begin());
    op = 1;
  } else if (kind == GPEMU_DIAG_INDICATOR_LE) {
    GP_TRY(diag_quantile(h, prob, par.data()));
    op = 2;
  }
  if (op) GP_TRY(upload(dpar, par.data(), d, st));
  diag_path_count(GPEMU_DIAG_PATH_TRANSFORM);
  hipLaunchKernelGGL(diag_split_kernel, dim3((unsigned)((N * S + 255) / 256)), dim3(256), 0, st, h->src, h->step_stride, h->n,
                     N, h->nw, d, op, dpar, h->Y);
  GP_HIP(hipGetLastError());
  if (kind == GPEMU_DIAG_RANK_Z || kind == GPEMU_DIAG_FOLDED_RANK_Z)
    GP_TRY(rank_rows(h->Y, d, N * K, 1, d, h->Y, 1, d, true, h->workspace_bytes, st));
  // the split chains' moments: means, then centred squares in the same chunks, then the sums over the chains
  int64_t tchunk = 0;
  const int nchunk = diag_chunks(h, &tchunk);
  const size_t need_part = sizeof(double) * (size_t)nchunk * (size_t)S;
  GP_TRY(dev_reserve(&h->part_bytes, need_part, {st}, {dev_field_bytes(&h->part, need_part)}));
  const unsigned gs = (unsigned)((S + 255) / 256);
  hipLaunchKernelGGL(acf_sum_kernel, dim3(gs, 1, (unsigned)nchunk), dim3(256), 0, st, h->Y, N, S, S, tchunk, h->part);
  hipLaunchKernelGGL(acf_mean_kernel, dim3(gs), dim3(256), 0, st, h->part, N, S, nchunk, h->mean);
  hipLaunchKernelGGL(diag_ss_kernel, dim3(gs, 1, (unsigned)nchunk), dim3(256), 0, st, h->Y, h->mean, N, S, tchunk, h->part);
  hipLaunchKernelGGL(acf_mean_kernel, dim3(gs), dim3(256), 0, st, h->part, N - 1, S, nchunk, h->var);
  double *dmom = h->small + d;   // grand mean | W | b
  hipLaunchKernelGGL(diag_chain_reduce_kernel, dim3(1, (unsigned)d), dim3(256), 0, st, h->mean, S, d, K,
                     (const double *)nullptr, 1.0 / (double)K, dmom);
  hipLaunchKernelGGL(diag_chain_reduce_kernel, dim3(1, (unsigned)d), dim3(256), 0, st, h->var, S, d, K,
                     (const double *)nullptr, 1.0 / (double)K, dmom + d);
  hipLaunchKernelGGL(diag_chain_reduce_kernel, dim3(1, (unsigned)d), dim3(256), 0, st, h->mean, S, d, K,
                     (const double *)dmom, 1.0 / (double)(K - 1), dmom + 2 * d);
  GP_HIP(hipGetLastError());
  std::vector<double> mom((size_t)3 * d);
  GP_HIP(hipMemcpyAsync(mom.data(), dmom, sizeof(double) * 3 * (size_t)d, hipMemcpyDeviceToHost, st));
  GP_HIP(hipStreamSynchronize(st));
  std::copy(mom.begin(), mom.begin() + d, grand_mean);
  std::copy(mom.begin() + d, mom.begin() + 2 * d, mean_var);
  std::copy(mom.begin() + 2 * d, mom.end(), var_of_means);
  h->kind = kind;
  return GPEMU_OK;
}

int gpemu_diag_range(gpemu_diag *h, double *min, double *max) {
  GP_ARG(h && min && max, "null pointer");
  GP_TRY(diag_fresh(h));
  if (h->kind < 0) { set_error("gpemu_diag_range before gpemu_diag_transform"); return GPEMU_ERR_STATE; }
  GP_HIP(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const int d = h->d;
  const int64_t count = h->N * h->K;
  const int nch = (int)std::min<int64_t>(DIAG_RANGE_CHUNKS, (count + 255) / 256);
  double *pmin = h->small + 8 * d, *pmax = pmin + (int64_t)DIAG_RANGE_CHUNKS * d, *dout = h->small + 4 * d;
  hipLaunchKernelGGL(diag_range_kernel, dim3((unsigned)d, (unsigned)nch), dim3(256), 0, st, h->Y, h->Y, count, d, pmin, pmax);
  hipLaunchKernelGGL(diag_range_kernel, dim3((unsigned)d, 1), dim3(256), 0, st, pmin, pmax, (int64_t)nch, d, dout, dout + d);
  GP_HIP(hipGetLastError());
  std::vector<double> r((size_t)2 * d);
  GP_HIP(hipMemcpyAsync(r.data(), dout, sizeof(double) * 2 * (size_t)d, hipMemcpyDeviceToHost, st));
  GP_HIP(hipStreamSynchronize(st));
  std::copy(r.begin(), r.begin() + d, min);
  std::copy(r.begin() + d, r.end(), max);
  return GPEMU_OK;
}

int gpemu_diag_series(gpemu_diag *h, double *Y_out) {
  GP_ARG(h && Y_out, "null pointer");
  GP_TRY(diag_fresh(h));
  if (h->kind < 0) { set_error("gpemu_diag_series before gpemu_diag_transform"); return GPEMU_ERR_STATE; }
  GP_HIP(hipSetDevice(h->device));
  GP_HIP(hipMemcpyAsync(Y_out, h->Y, sizeof(double) * (size_t)(h->N * h->S), hipMemcpyDeviceToHost, h->stream));
  GP_HIP(hipStreamSynchronize(h->stream));
  return GPEMU_OK;
}

int gpemu_diag_acov(gpemu_diag *h, int64_t lag0, int64_t n_lags, double *g_out) {
  GP_ARG(h && g_out, "null pointer");
  GP_ARG(lag0 >= 0 && n_lags >= 1 && n_lags <= 4096 && lag0 % ACF_LPT == 0, "lag block (lag0 must be a multiple of 16)");
  GP_ARG(n_lags <= h->N && lag0 <= h->N - n_lags, "lags beyond the split chains' length");
  GP_TRY(diag_fresh(h));
  if (h->kind < 0) { set_error("gpemu_diag_acov before gpemu_diag_transform"); return GPEMU_ERR_STATE; }
  GP_ARG(lag0 == 0 || h->acov_started, "the first block after a transform must start at lag 0");
  GP_HIP(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const int d = h->d;
  const int64_t N = h->N, S = h->S;
  int64_t tchunk = 0;
  const int nchunk = diag_chunks(h, &tchunk);
  const int nlg = (int)((n_lags + ACF_LPT - 1) / ACF_LPT);
  const size_t need_part = sizeof(double) * (size_t)nchunk * (size_t)n_lags * (size_t)S;
  const size_t need_acf = sizeof(double) * (size_t)n_lags * (size_t)S;
  GP_TRY(dev_reserve(&h->part_bytes, need_part, {st}, {dev_field_bytes(&h->part, need_part)}));
  GP_TRY(dev_reserve(&h->acf_bytes, need_acf, {st}, {dev_field_bytes(&h->acf, need_acf)}));
  diag_path_count(GPEMU_DIAG_PATH_ACOV_BLOCK);
  const unsigned gs = (unsigned)((S + 255) / 256);
  hipLaunchKernelGGL(acf_lag_kernel, dim3(gs, (unsigned)nlg, (unsigned)nchunk), dim3(256), 0, st, h->Y, h->mean, N, S, S,
                     tchunk, lag0, (int)n_lags, h->part);
  hipLaunchKernelGGL(acf_reduce_kernel, dim3(gs, (unsigned)n_lags), dim3(256), 0, st, h->part, S, (int)n_lags, nchunk, h->acf,
                     h->acf0, lag0 == 0 ? 1 : 0);
  DevScope sc(st);
  double *dg = nullptr;
  GP_TRY(sc.alloc(&dg, n_lags * d));
  hipLaunchKernelGGL(diag_chain_reduce_kernel, dim3((unsigned)n_lags, (unsigned)d), dim3(256), 0, st, h->acf, S, d, h->K,
                     (const double *)nullptr, 1.0 / ((double)h->K * (double)N), dg);
  GP_HIP(hipGetLastError());
  GP_TRY(sc.download(g_out, dg, n_lags * d));
  GP_HIP(hipStreamSynchronize(st));
  h->acov_started = true;
  return GPEMU_OK;
}

}  // extern "C"
