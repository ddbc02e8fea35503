// Exact order statistics of many rows at once (gpemu_select*) and the posterior-predictive reduction built on them
// (gpemu_posterior_predictive*).
//
// Selection: the radix select of k_select.hip (select_rows of rows_dev.h) without weights: rank r is the
// target r + 1 under unit weights.  An element of the input, not an approximation; a row with a NaN returns NaN for every
// rank (np.quantile); -0 and +0 are distinct keys next to each other, so either may be returned for a zero.  Rows go in
// batches of SEL_ROWS.
//
// Posterior predictive: PC means / variances of all S rows through gpemu_gp_predict_dev in fixed chunks of PP_CHUNK
// logical rows (a chunk that is not contiguous in the caller's block layout is gathered into a staging buffer first, so
// the launches -- and the bits -- are those of the contiguous rows), then per block of features
//   pp_project_kernel  mu[f][s] = (sum_p mean[s][p] comp[p][f]) scale_f + mean_f, feature-major (cv_backproject's sum);
//   pp_rowsum_kernel   sums of fixed 4096-sample chunks (lane-strided partial sums in index order, tree B of wg_dev.h),
//   pp_finish_kernel   added in chunk order: the mean, then the centred second moment (two passes);
//   selection on the rows of the workspace.
// var_emu_f = mean_s sigma^2_f(theta_s) = (sum_p comp[p][f] vbar_p comp[p][f] + cov_unexplained[f][f]) scale_f^2 with
// vbar_p = mean_s var_p(theta_s): the mean is linear and every term is non-negative, so the F x S variances never exist.
// Every sum over samples runs over chunks fixed by the logical sample index: the bits do not depend on the workspace,
// on the feature blocks or on the run.
//
// gpemu_posterior_predictive_weighted*  is the same reduction (pp_reduce) under rows of fixed-point weights:
// the sums by weighted_rowmean of k_wsummary.hip, in the same tree, the quantiles by the weighted select.
#include <algorithm>
#include <vector>

#include "internal.h"
#include "rows_dev.h"
#include "sampler_internal.h"
#include "wg_dev.h"

namespace gpemu {

constexpr int64_t PP_CHUNK = 2048;   // logical rows per predict pass (one pass of gpemu_gp_predict_dev)
constexpr int64_t PP_SUM = 4096;     // samples per partial sum
constexpr int PP_FT = 32;            // features per projection workgroup
constexpr int64_t PP_FIXED = GPEMU_POSTPRED_FIXED_BYTES;

// out[r n_ranks + i] = order statistic ranks[i] of row r (elements dV[r row_stride + j elem_stride], j < S): the radix
// select of k_select.hip without weights, target rank + 1, all on st; synchronises st before it returns.  The caller has
// validated the ranks.
static int select_ranks(const double *dV, int64_t R, int64_t S, int64_t row_stride, int64_t elem_stride, int64_t n_ranks,
                        const int64_t *ranks, double *dout, hipStream_t st) {
  std::vector<u64> targets((size_t)n_ranks);
  for (int64_t i = 0; i < n_ranks; ++i) targets[(size_t)i] = (u64)ranks[i] + 1;
  return select_rows(dV, R, S, row_stride, elem_stride, 1, nullptr, 0, n_ranks, targets.data(), dout,
                     std::min<int64_t>(R, SEL_ROWS), [] { postpred_path_count(GPEMU_POSTPRED_PATH_SELECT_PASS); }, st);
}

static int select_check(int64_t R, int64_t S, int64_t n_ranks, const int64_t *ranks) {
  GP_ARG(R > 0, "R must be positive");
  GP_ARG(S > 0, "S must be positive");
  GP_ARG(n_ranks > 0 && ranks, "n_ranks must be positive");
  for (int64_t i = 0; i < n_ranks; ++i) GP_ARG(ranks[i] >= 0 && ranks[i] < S, "every rank must be in [0, S)");
  return GPEMU_OK;
}

// ---- posterior predictive ------------------------------------------------------------------------------------------
// workgroup (256 samples, PP_FT features): W[(f - f0) ldw + s] = central value of feature f for sample s
__global__ __launch_bounds__(256) void pp_project_kernel(const double *__restrict__ M, int64_t S, int k,
                                                         const double *__restrict__ comp,
                                                         const double *__restrict__ smean,
                                                         const double *__restrict__ sscale, int64_t F, int64_t f0,
                                                         int64_t fb, double *__restrict__ W, int64_t ldw) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ft0 = f0 + (int64_t)blockIdx.y * PP_FT;
  const int nf = (int)((f0 + fb - ft0 < PP_FT) ? f0 + fb - ft0 : PP_FT);
  if (s >= S) return;
  double a[PP_FT];
#pragma unroll
  for (int j = 0; j < PP_FT; ++j) a[j] = 0.0;
  const double *mrow = M + s * k;
  for (int p = 0; p < k; ++p) {
    const double mp = mrow[p];
    const double *c = comp + (int64_t)p * F + ft0;   // the same for the whole workgroup
#pragma unroll
    for (int j = 0; j < PP_FT; ++j)
      if (j < nf) a[j] = fma(mp, c[j], a[j]);
  }
#pragma unroll
  for (int j = 0; j < PP_FT; ++j)
    if (j < nf) W[(ft0 - f0 + j) * ldw + s] = a[j] * sscale[ft0 + j] + smean[ft0 + j];
}

// part[row nchunk + c] = sum over samples [c PP_SUM, (c + 1) PP_SUM) of x (centre null) or (x - centre[row])^2,
// x = X[row rs + i es]: every lane adds its 16 elements in index order, then tree B of wg_dev.h
__global__ __launch_bounds__(256) void pp_rowsum_kernel(const double *__restrict__ X, int64_t rs, int64_t es, int64_t S,
                                                        const double *__restrict__ centre, double *__restrict__ part,
                                                        int64_t nchunk) {
  __shared__ double ws[4];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x, row = blockIdx.y;
  const double *x = X + row * rs;
  const double mu = centre ? centre[row] : 0.0;
  double acc = 0.0;
  for (int j = 0; j < PP_SUM / 256; ++j) {
    const int64_t i = c * PP_SUM + (int64_t)j * 256 + tid;
    if (i < S) {
      const double v = x[i * es];
      acc += centre ? (v - mu) * (v - mu) : v;
    }
  }
  acc = wg_sum_b<4>(acc, ws);
  if (tid == 0) part[row * nchunk + c] = acc;
}

// out[row] = (sum of the row's partial sums, in chunk order) * scale
__global__ __launch_bounds__(256) void pp_finish_kernel(const double *__restrict__ part, int64_t R, int64_t nchunk,
                                                        double scale, double *__restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= R) return;
  double acc = 0.0;
  for (int64_t c = 0; c < nchunk; ++c) acc += part[row * nchunk + c];
  out[row] = acc * scale;
}

// var_emu[f] = (sum_p comp[p][f] vbar_p comp[p][f] + cov_unexplained[f][f]) scale_f^2  (cv_backproject's variance sum)
__global__ __launch_bounds__(256) void pp_varemu_kernel(const double *__restrict__ vbar, const double *__restrict__ comp,
                                                        const double *__restrict__ sscale,
                                                        const double *__restrict__ cunexpl, int k, int64_t F,
                                                        double *__restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  double b = 0.0;
  for (int p = 0; p < k; ++p) {
    const double c = comp[(int64_t)p * F + f];
    b = fma(c * vbar[p], c, b);
  }
  const double sc = sscale[f];
  out[f] = (b + cunexpl[f * F + f]) * (sc * sc);
}

static int launch_rowmean(const double *X, int64_t rs, int64_t es, int64_t R, int64_t S, const double *centre,
                          double *part, double *out, hipStream_t st) {
  const int64_t nchunk = (S + PP_SUM - 1) / PP_SUM;
  for (int64_t r0 = 0; r0 < R; r0 += 32768) {   // grid.y
    const int64_t nr = std::min<int64_t>(32768, R - r0);
    hipLaunchKernelGGL(pp_rowsum_kernel, dim3((unsigned)nchunk, (unsigned)nr), dim3(256), 0, st, X + r0 * rs, rs, es, S,
                       centre ? centre + r0 : nullptr, part + r0 * nchunk, nchunk);
    GP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(pp_finish_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, part, R, nchunk,
                     1.0 / (double)S, out);
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_postpred_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_POSTPRED, out, n); }

int gpemu_select_dev(int device, int64_t R, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                     int64_t n_ranks, const int64_t *ranks, double *dout, void *stream) {
  GP_ARG(dV && dout, "null pointer");
  GP_TRY(select_check(R, S, n_ranks, ranks));
  GP_ARG(row_stride > 0 && elem_stride > 0, "strides must be positive");
  GP_TRY(device_ready(device));
  return select_ranks(dV, R, S, row_stride, elem_stride, n_ranks, ranks, dout, (hipStream_t)stream);
}

int gpemu_select(int device, int64_t R, int64_t S, const double *V, int64_t n_ranks, const int64_t *ranks, double *out) {
  GP_ARG(V && out, "null pointer");
  GP_TRY(select_check(R, S, n_ranks, ranks));
  return with_host_rows(device, R, S, V, n_ranks, out, [&](const double *dV, double *dout, hipStream_t st) {
    return select_ranks(dV, R, S, S, 1, n_ranks, ranks, dout, st);
  });
}

}  // extern "C"

// the fixed-point weights of gpemu_posterior_predictive_weighted*: R_w rows, n_sel targets each
struct PpWeights {
  int64_t R_w;
  const u64 *dq;       // [R_w][ldq], device
  int64_t ldq;
  const u64 *targets;  // [R_w][n_sel], host
};

// The reduction of both families over validated rows, on st (waited for).  wt null: the sample counts 1 and n_sel ranks
// select; the outputs are [F] (dsel [F][n_sel]).  Else every sum runs under each weight row (weighted_rowmean of
// rows_dev.h, the same tree), n_sel targets per weight row select, and the outputs are [R_w][F] (dsel [R_w][F][n_sel])
static int pp_reduce(gpemu_model *m, const RowsView &X, int64_t n_sel, const int64_t *ranks, const PpWeights *wt,
                     int64_t workspace_bytes, double *dmean, double *dvar_param, double *dvar_emu, double *dsel,
                     hipStream_t st) {
  const double *dX = X.base;
  const int64_t block_rows = X.block_rows, S = X.rows(), F = m->F, k = m->k, d = m->d, n_ranks = n_sel;
  const int64_t R_w = wt ? wt->R_w : 1;

  // the plan: the PC arrays stay resident, the features go through the workspace in blocks
  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t pc_bytes = 2 * S * k * 8;
  const bool want_ws = dmean || dvar_param || n_ranks > 0;
  int64_t Fb = F;
  if (want_ws) {
    const int64_t room = budget - pc_bytes - PP_FIXED;
    Fb = room > 0 ? std::min<int64_t>(F, room / (8 * S)) : 0;
    if (Fb < F) Fb = Fb / 16 * 16;
    if (Fb < std::min<int64_t>(F, 16)) {
      set_error("posterior_predictive: out of memory: %lld rows need %lld bytes of PC arrays, %lld bytes of scratch and "
                "%lld bytes for one block of 16 features; %lld bytes %s", (long long)S, (long long)pc_bytes,
                (long long)PP_FIXED, (long long)(std::min<int64_t>(F, 16) * 8 * S), (long long)budget,
                workspace_budget_name(workspace_bytes));
      return GPEMU_ERR_HIP;
    }
  }
  const int64_t nchunk = (S + PP_SUM - 1) / PP_SUM;

  DevScope sc(st);
  double *Mpc = nullptr, *Vpc = nullptr, *stage = nullptr, *W = nullptr, *part = nullptr, *vbar = nullptr, *mu = nullptr;
  GP_TRY(sc.alloc(&Mpc, S * k));
  GP_TRY(sc.alloc(&Vpc, S * k));
  if (!X.dense()) GP_TRY(sc.alloc(&stage, PP_CHUNK * d));
  u64 *dQ = nullptr;
  GP_TRY(sc.alloc(&part, R_w * std::max(Fb, k) * nchunk));
  GP_TRY(sc.alloc(&vbar, R_w * k));
  GP_TRY(sc.alloc(&mu, R_w * F));
  if (wt) {
    GP_TRY(sc.alloc(&dQ, R_w));
    GP_TRY(weight_totals(wt->dq, wt->ldq, R_w, S, dQ, st));
  }
  if (want_ws) GP_TRY(sc.alloc(&W, Fb * S));

  for (int64_t r0 = 0; r0 < S; r0 += PP_CHUNK) {
    const int64_t nb = std::min(PP_CHUNK, S - r0);
    const double *src = stage;
    if (X.dense())
      src = dX + r0 * d;
    else if (r0 / block_rows == (r0 + nb - 1) / block_rows)   // the chunk lies within one block
      src = X.row(r0);
    else
      GP_TRY(gather_rows(X, r0, nb, stage, st));
    GP_TRY(gpemu_gp_predict_dev(m, nb, src, Mpc + r0 * k, Vpc + r0 * k, st));
  }

  if (dvar_emu) {
    if (wt)
      GP_TRY(weighted_rowmean(Vpc, 1, k, k, S, R_w, wt->dq, wt->ldq, dQ, nullptr, 0, part, k, vbar, k, st));
    else
      GP_TRY(launch_rowmean(Vpc, 1, k, k, S, nullptr, part, vbar, st));
    for (int64_t w = 0; w < R_w; ++w)
      hipLaunchKernelGGL(pp_varemu_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, vbar + w * k, m->comp,
                         m->sscale, m->cunexpl, (int)k, F, dvar_emu + w * F);
    GP_HIP(hipGetLastError());
  }
  if (want_ws) {
    if (wt)
      wsummary_path_count(Fb >= F ? GPEMU_WSUMMARY_PATH_BANDS_WHOLE : GPEMU_WSUMMARY_PATH_BANDS_FEATURE_BLOCKED);
    else
      postpred_path_count(Fb >= F ? GPEMU_POSTPRED_PATH_WHOLE : GPEMU_POSTPRED_PATH_FEATURE_BLOCKED);
    for (int64_t f0 = 0; f0 < F; f0 += Fb) {
      const int64_t fb = std::min(Fb, F - f0);
      if (!wt) postpred_path_count(GPEMU_POSTPRED_PATH_FEATURE_BLOCK);
      hipLaunchKernelGGL(pp_project_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)((fb + PP_FT - 1) / PP_FT)),
                         dim3(256), 0, st, Mpc, S, (int)k, m->comp, m->smean, m->sscale, F, f0, fb, W, S);
      GP_HIP(hipGetLastError());
      if (!wt) {
        if (dmean || dvar_param) GP_TRY(launch_rowmean(W, S, 1, fb, S, nullptr, part, mu + f0, st));
        if (dvar_param) GP_TRY(launch_rowmean(W, S, 1, fb, S, mu + f0, part, dvar_param + f0, st));
        if (n_ranks > 0) GP_TRY(select_ranks(W, fb, S, S, 1, n_ranks, ranks, dsel + f0 * n_ranks, st));
        continue;
      }
      if (dmean || dvar_param)
        GP_TRY(weighted_rowmean(W, S, 1, fb, S, R_w, wt->dq, wt->ldq, dQ, nullptr, 0, part, Fb, mu + f0, F, st));
      if (dvar_param)
        GP_TRY(weighted_rowmean(W, S, 1, fb, S, R_w, wt->dq, wt->ldq, dQ, mu + f0, F, part, Fb, dvar_param + f0, F, st));
      for (int64_t w = 0; n_sel > 0 && w < R_w; ++w)   // a weight row at a time: its rows of dsel are contiguous
        GP_TRY(select_rows(W, fb, S, S, 1, 1, wt->dq + w * wt->ldq, wt->ldq, n_sel, wt->targets + w * n_sel,
                           dsel + (w * F + f0) * n_sel, std::min<int64_t>(fb, SEL_ROWS),
                           [] { wsummary_path_count(GPEMU_WSUMMARY_PATH_SELECT_PASS); }, st));
    }
    if (dmean) GP_HIP(hipMemcpyAsync(dmean, mu, sizeof(double) * (size_t)(R_w * F), hipMemcpyDeviceToDevice, st));
  }
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

// the rows of a posterior-predictive _dev call as a view, with the checks the two families share
static int pp_view(gpemu_model *m, const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows,
                   int64_t workspace_bytes, RowsView *X) {
  GP_ARG(m && dX, "null pointer");
  *X = RowsView{dX, n_blocks, block_rows, block_stride_rows * m->d, (int)m->d};
  GP_TRY(rows_check(*X));
  GP_ARG(n_blocks <= INT64_MAX / block_rows, "n_blocks * block_rows overflows");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  return GPEMU_OK;
}

static int ppw_check(int64_t S, int64_t R_w, int64_t n_targets, const uint64_t *targets, const void *quantiles) {
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(R_w >= 1 && R_w <= WS_MAX_RW, "R_w must be in [1, 64]");
  GP_ARG(n_targets >= 0 && n_targets < (1ll << 24), "n_targets must be in [0, 2^24)");
  if (n_targets > 0) {
    GP_ARG(targets && quantiles, "targets or quantiles is null with n_targets > 0");
    for (int64_t i = 0; i < R_w * n_targets; ++i)
      GP_ARG(targets[i] >= 1 && targets[i] <= (1ull << 53), "every target must be in [1, 2^53]");
  }
  return GPEMU_OK;
}

extern "C" {

int gpemu_posterior_predictive_dev(gpemu_model *m, const double *dX, int64_t n_blocks, int64_t block_rows,
                                   int64_t block_stride_rows, int64_t n_ranks, const int64_t *ranks,
                                   int64_t workspace_bytes, double *dmean, double *dvar_param, double *dvar_emu,
                                   double *dorder, void *stream) {
  RowsView X;
  GP_TRY(pp_view(m, dX, n_blocks, block_rows, block_stride_rows, workspace_bytes, &X));
  GP_ARG(n_ranks >= 0, "n_ranks must be >= 0");
  if (n_ranks > 0) {
    GP_ARG(dorder, "order_stats is null with n_ranks > 0");
    GP_TRY(select_check(m->F, X.rows(), n_ranks, ranks));
  }
  GP_HIP(hipSetDevice(m->device));
  return pp_reduce(m, X, n_ranks, ranks, nullptr, workspace_bytes, dmean, dvar_param, dvar_emu, dorder,
                   stream ? (hipStream_t)stream : m->stream);
}

int gpemu_posterior_predictive_weighted_dev(gpemu_model *m, const double *dX, int64_t n_blocks, int64_t block_rows,
                                            int64_t block_stride_rows, int64_t R_w, const uint64_t *dq, int64_t ldq,
                                            int64_t n_targets, const uint64_t *targets, double *dmean,
                                            double *dvar_param, double *dvar_emu, double *dquantiles,
                                            const gpemu_call_ctx *ctx) {
  RowsView X;
  GP_TRY(pp_view(m, dX, n_blocks, block_rows, block_stride_rows, ctx_workspace(ctx), &X));
  GP_ARG(dq, "null pointer");
  GP_TRY(ppw_check(X.rows(), R_w, n_targets, targets, dquantiles));
  GP_ARG(ldq >= X.rows(), "ldq must be at least the number of rows");
  GP_HIP(hipSetDevice(m->device));
  const PpWeights wt{R_w, (const u64 *)dq, ldq, (const u64 *)targets};
  return pp_reduce(m, X, n_targets, nullptr, &wt, ctx_workspace(ctx), dmean, dvar_param, dvar_emu, dquantiles,
                   ctx_stream(ctx) ? ctx_stream(ctx) : m->stream);
}

int gpemu_posterior_predictive_weighted(gpemu_model *m, int64_t S, const double *X, int64_t R_w, const uint64_t *q,
                                        int64_t n_targets, const uint64_t *targets, int64_t workspace_bytes,
                                        double *mean, double *var_param, double *var_emu, double *quantiles) {
  GP_ARG(m && X && q, "null pointer");
  GP_TRY(ppw_check(S, R_w, n_targets, targets, quantiles));
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  for (int64_t i = 0; i < S * m->d; ++i) GP_ARG(std::isfinite(X[i]), "X contains NaN or infinity");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int64_t F = m->F;
  DevScope sc(st);
  double *dX = nullptr, *dm = nullptr, *dvp = nullptr, *dve = nullptr, *dqt = nullptr;
  u64 *dq = nullptr;
  GP_TRY(sc.alloc(&dX, S * m->d));
  GP_TRY(sc.alloc(&dq, R_w * S));
  if (mean) GP_TRY(sc.alloc(&dm, R_w * F));
  if (var_param) GP_TRY(sc.alloc(&dvp, R_w * F));
  if (var_emu) GP_TRY(sc.alloc(&dve, R_w * F));
  if (n_targets > 0) GP_TRY(sc.alloc(&dqt, R_w * F * n_targets));
  GP_TRY(upload(dX, X, S * m->d, st));
  GP_TRY(upload(dq, (const u64 *)q, R_w * S, st));
  const gpemu_call_ctx ctx{st, workspace_bytes};
  GP_TRY(gpemu_posterior_predictive_weighted_dev(m, dX, 1, S, S, R_w, (const uint64_t *)dq, S, n_targets, targets, dm, dvp, dve, dqt, &ctx));
  if (mean) GP_TRY(sc.download(mean, dm, R_w * F));
  if (var_param) GP_TRY(sc.download(var_param, dvp, R_w * F));
  if (var_emu) GP_TRY(sc.download(var_emu, dve, R_w * F));
  if (n_targets > 0) GP_TRY(sc.download(quantiles, dqt, R_w * F * n_targets));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_posterior_predictive(gpemu_model *m, int64_t S, const double *X, int64_t n_ranks, const int64_t *ranks,
                               int64_t workspace_bytes, double *mean, double *var_param, double *var_emu,
                               double *order_stats) {
  GP_ARG(m && X, "null pointer");
  GP_ARG(S > 0, "S must be positive");
  GP_ARG(n_ranks >= 0, "n_ranks must be >= 0");
  GP_ARG(n_ranks == 0 || order_stats, "order_stats is null with n_ranks > 0");
  for (int64_t i = 0; i < S * m->d; ++i) GP_ARG(std::isfinite(X[i]), "X contains NaN or infinity");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int64_t F = m->F;
  DevScope sc(st);
  double *dX = nullptr, *dm = nullptr, *dvp = nullptr, *dve = nullptr, *dq = nullptr;
  GP_TRY(sc.alloc(&dX, S * m->d));
  if (mean) GP_TRY(sc.alloc(&dm, F));
  if (var_param) GP_TRY(sc.alloc(&dvp, F));
  if (var_emu) GP_TRY(sc.alloc(&dve, F));
  if (n_ranks > 0) GP_TRY(sc.alloc(&dq, F * n_ranks));
  GP_TRY(upload(dX, X, S * m->d, st));
  GP_TRY(gpemu_posterior_predictive_dev(m, dX, 1, S, S, n_ranks, ranks, workspace_bytes, dm, dvp, dve, dq, st));
  if (mean) GP_TRY(sc.download(mean, dm, F));
  if (var_param) GP_TRY(sc.download(var_param, dvp, F));
  if (var_emu) GP_TRY(sc.download(var_emu, dve, F));
  if (n_ranks > 0) GP_TRY(sc.download(order_stats, dq, F * n_ranks));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_sampler_chain_ptr(gpemu_sampler *s, int64_t first, const double **dchain, int64_t *n_steps) {
  GP_ARG(s && dchain && n_steps, "null pointer");
  GP_ARG(first >= 0 && first <= s->chain_len, "first must be in [0, chain_len]");
  GP_HIP(hipSetDevice(s->device));
  GP_HIP(hipStreamSynchronize(s->stream));   // the steps stored so far are in the buffer
  *dchain = s->chain + first * s->W * s->d;
  *n_steps = s->chain_len - first;
  return GPEMU_OK;
}

}  // extern "C"
