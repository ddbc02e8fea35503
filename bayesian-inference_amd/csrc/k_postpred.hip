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

int gpemu_posterior_predictive_dev(gpemu_model *m, const double *dX, int64_t n_blocks, int64_t block_rows,
                                   int64_t block_stride_rows, int64_t n_ranks, const int64_t *ranks,
                                   int64_t workspace_bytes, double *dmean, double *dvar_param, double *dvar_emu,
                                   double *dorder, void *stream) {
  GP_ARG(m && dX, "null pointer");
  const RowsView X{dX, n_blocks, block_rows, block_stride_rows * m->d, (int)m->d};
  GP_TRY(rows_check(X));
  GP_ARG(n_blocks <= INT64_MAX / block_rows, "n_blocks * block_rows overflows");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_ARG(n_ranks >= 0, "n_ranks must be >= 0");
  const int64_t S = n_blocks * block_rows, F = m->F, k = m->k, d = m->d;
  if (n_ranks > 0) {
    GP_ARG(dorder, "order_stats is null with n_ranks > 0");
    GP_TRY(select_check(F, S, n_ranks, ranks));
  }
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;

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
  GP_TRY(sc.alloc(&part, std::max(Fb, k) * nchunk));
  GP_TRY(sc.alloc(&vbar, k));
  GP_TRY(sc.alloc(&mu, F));
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
    GP_TRY(launch_rowmean(Vpc, 1, k, k, S, nullptr, part, vbar, st));
    hipLaunchKernelGGL(pp_varemu_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, vbar, m->comp, m->sscale,
                       m->cunexpl, (int)k, F, dvar_emu);
    GP_HIP(hipGetLastError());
  }
  if (want_ws) {
    postpred_path_count(Fb >= F ? GPEMU_POSTPRED_PATH_WHOLE : GPEMU_POSTPRED_PATH_FEATURE_BLOCKED);
    for (int64_t f0 = 0; f0 < F; f0 += Fb) {
      const int64_t fb = std::min(Fb, F - f0);
      postpred_path_count(GPEMU_POSTPRED_PATH_FEATURE_BLOCK);
      hipLaunchKernelGGL(pp_project_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)((fb + PP_FT - 1) / PP_FT)),
                         dim3(256), 0, st, Mpc, S, (int)k, m->comp, m->smean, m->sscale, F, f0, fb, W, S);
      GP_HIP(hipGetLastError());
      if (dmean || dvar_param) GP_TRY(launch_rowmean(W, S, 1, fb, S, nullptr, part, mu + f0, st));
      if (dvar_param) GP_TRY(launch_rowmean(W, S, 1, fb, S, mu + f0, part, dvar_param + f0, st));
      if (n_ranks > 0) GP_TRY(select_ranks(W, fb, S, S, 1, n_ranks, ranks, dorder + f0 * n_ranks, st));
    }
    if (dmean) GP_HIP(hipMemcpyAsync(dmean, mu, sizeof(double) * (size_t)F, hipMemcpyDeviceToDevice, st));
  }
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
