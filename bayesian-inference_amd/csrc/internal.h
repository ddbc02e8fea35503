// Internal declarations shared by the translation units of libgpemu.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/gpemu.h"

namespace gpemu {

// ---- error plumbing -------------------------------------------------------------------------
void set_error(const char *fmt, ...);
#define GP_HIP(call)                                                                        \
  do {                                                                                      \
    hipError_t e__ = (call);                                                                \
    if (e__ != hipSuccess) {                                                                \
      gpemu::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__,    \
                       __LINE__);                                                           \
      return GPEMU_ERR_HIP;                                                                 \
    }                                                                                       \
  } while (0)
#define GP_ARG(cond, msg)                \
  do {                                   \
    if (!(cond)) {                       \
      gpemu::set_error("bad argument: %s", msg); \
      return GPEMU_ERR_ARG;              \
    }                                    \
  } while (0)
// propagate a non-OK status code of a library call
#define GP_TRY(expr)                     \
  do {                                   \
    const int rc__ = (expr);             \
    if (rc__ != GPEMU_OK) return rc__;   \
  } while (0)

// lets `fn` (a kernel, by its host stub) use `bytes` of dynamic LDS beyond the default 64 KiB: the attribute is set once
// per (function, current device), under a lock, so that later calls -- from any host thread -- make no call to set it
int allow_dynamic_lds(const void *fn, int bytes);

// GPEMU_ERR_NO_DEVICE without a HIP device, GPEMU_ERR_ARG for a `device` that is none of them; else makes it current
int device_ready(int device);

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// one relaxed host-side increment per launch decision, in one table (gpemu_api.hip) with a row per family of gpemu.h;
// a path outside its family's enum is not counted
enum PathFamily { PATHS_LOGPOST, PATHS_FIT, PATHS_WIDE, PATHS_SRC, PATHS_GRAD, PATHS_POSTPRED, PATHS_HMC, PATHS_DIAG,
                  PATHS_SOBOL, PATHS_MARGINAL, PATHS_DESIGN, PATHS_KDE2D, PATHS_LOO, PATHS_KNN, PATHS_PAIRLSE,
                  PATHS_REWEIGHT, PATHS_WSUMMARY, PATHS_SOBOL_PAIRS, PATH_FAMILIES };
void count_path(PathFamily family, int path);
int read_path_counts(PathFamily family, int64_t *out, int64_t n);     // what the eighteen public gpemu_*_path_counts return
static inline void path_count(int path) { count_path(PATHS_LOGPOST, path); }    // enum gpemu_path
static inline void fit_path_count(int path) { count_path(PATHS_FIT, path); }    // enum gpemu_fit_path
static inline void wide_path_count(int path) { count_path(PATHS_WIDE, path); }  // enum gpemu_wide_path: d > 8 only
static inline void src_path_count(int path) { count_path(PATHS_SRC, path); }    // enum gpemu_src_path
static inline void grad_path_count(int path) { count_path(PATHS_GRAD, path); }  // enum gpemu_grad_path
static inline void postpred_path_count(int path) { count_path(PATHS_POSTPRED, path); }  // enum gpemu_postpred_path
static inline void wsummary_path_count(int path) { count_path(PATHS_WSUMMARY, path); }  // enum gpemu_wsummary_path

constexpr int DPAD = 8;        // parameter dimensions padded to 8 (reference uses d = 6 or 7) ...
constexpr int DPAD_WIDE = 16;  // ... or, for 9 <= d <= 16, to 16 (separate instantiations: d <= 8 keeps the code of DPAD)
// padded width of a d-parameter model, fit handle or sampler: the row stride of every padded layout
__host__ __device__ inline int dpad_of(int64_t d) { return d <= DPAD ? DPAD : DPAD_WIDE; }
constexpr int TILE = 128;      // row / column tile of the triangular GEMM
constexpr int KSTAR_ROWS_BIG = 64;    // training rows per workgroup of the cross-kernel: batches of more than 256 columns
constexpr int KSTAR_ROWS_SMALL = 32;  // ... and of at most KSTAR_SMALL_MAX
constexpr int KSTAR_SMALL_MAX = 128;  // (256 until round 4: at 129 .. 256 columns the 32-row form is 1 280 front workgroups against 768 resident)

// ---- device model -----------------------------------------------------------------------------
struct Workspace {
  int64_t Bcap = 0;            // padded batch capacity (multiple of TILE)
  double *Xq = nullptr;        // [Bcap][dp]     query points (padded with 0; dp: the model's padded width)
  double *KS = nullptr;        // [k][Npad][Bcap] cross-kernel K_*^T per PC
  double *mean_part = nullptr; // [Bcap][k][nchunk] partial K_* . alpha per 64- (or 32-) row chunk
  double *mean_part2 = nullptr; // second copy: the fused sampler run reads one half-step's while the next is written
  double *vsq_part = nullptr;  // [Bcap][k][nrb]    partial ||W k_*||^2 per 64- (or 32-) row block
  double *mean = nullptr;      // [Bcap][k]
  double *var = nullptr;       // [Bcap][k]
  double *logp = nullptr;      // [Bcap]
  int cur_nrb = 0;             // row blocks of vsq_part written by the last triangular GEMM launch
  int cur_nchunk = 0;          // row chunks of mean_part written by the last kstar launch
};

}  // namespace gpemu

struct gpemu_model {
  int device = 0;
  int64_t N = 0, d = 0, F = 0, k = 0;
  int dp = gpemu::DPAD;        // padded width of every [..][dp] layout below: dpad_of(d), 8 or 16
  int64_t Npad = 0;            // N rounded up to TILE
  int num_cu = 256;
  // LPT schedule of the persistent triangular GEMM for the current number of column tiles
  void *sched_items = nullptr; // TrmmItem[sched_workers][sched_max_items]
  int *sched_cnt = nullptr;    // [sched_workers]
  int sched_ncb = -1, sched_max_items = 0, sched_workers = 0;
  int sched_cap = 0;           // worker cap the current schedule was built for
  struct SchedEntry { int ncb, cap; void *items; int *cnt; int max_items, workers; };
  std::vector<SchedEntry> sched_cache;   // every schedule built so far (sched_items / sched_cnt point into one of them)
  // the sampler's compacted half-step (k_predict.hip: live_deal): for one launch shape, the GEMM's schedule and the
  // cross-kernel's workgroup map of EVERY number of live 64-column blocks, 0 .. 2 ncb, picked on the device
  struct LiveDeal { int ncb, cap, form; void *items; int *cnt; int *kmap; int max_items, workers, nwg; };
  std::vector<LiveDeal> live_cache;
  int64_t vsq_nrb = 0;         // row blocks of partial ||W k_*||^2 the triangular GEMM writes
  // schedule of the small-batch triangular GEMM (k_trmm_small.hip) for the current number of 32-column blocks
  void *sm_items = nullptr;
  int *sm_cnt = nullptr;
  int sm_ncb = -1, sm_max_items = 0, sm_workers = 0, sm_cap = 0;
  // every small-batch schedule built so far, keyed by (ncb, cap): the stand-alone launch (cap = num_cu) and the launch
  // shared with other groups (cap = -worker cap) alternate in a drop-in run (log_posterior(X) of a few rows between
  // sampler blocks), and a launch in flight keeps reading the one it was given -- so none is freed before the model is
  // (a few KB each; bounded: the oldest goes, after a stream sync, beyond 16)
  std::vector<SchedEntry> sm_cache;
  // likelihood with the observable blocks on different workgroups (k_loglik.hip: loglik_tasks_kernel): the terms' way
  // to the workgroup that adds them, and the tickets that tell which one that is
  double *lik_terms = nullptr;      // [lik_terms_cap][64]
  unsigned *lik_tickets = nullptr;  // [lik_terms_cap], zero between launches
  int64_t lik_terms_cap = 0;
  int kernel_kind = 0;
  double nu = 0;
  int has_const = 0, has_noise = 0;
  hipStream_t stream = nullptr;

  // per-PC GP state on the device
  // cross-kernel operands for the matrix cores (kstar_host.h; predict_dev.h: kstar_mfma_block)
  int ksteps = 2;              // MFMA k-steps of the augmented product: 4 ksteps >= d + 1 (2, 3 at dp 8; 3 .. 5 at dp 16)
  double *Xa = nullptr;        // [k][Npad/16][ksteps][64]  augmented, centred training rows in A-fragment order
  double *alf = nullptr;       // [k][Npad/16][16]          alpha in accumulator-row order
  double *qsc = nullptr;       // [k][4 ksteps]             query side: q' = q qsc + qof
  double *qof = nullptr;
  double *etab = nullptr;      // [2^KSTAR_TB]              2^(j / 2^KSTAR_TB)  (kind 4: + the MaternNu of nu)
  // Matern-0.5 and general nu < 1 only (the direct distance of near-coincident pairs): row-major scaled rows, else null
  double *Xs = nullptr;        // [k][Npad][dp]  X_train / ls_p  (padded rows/dims = 0)
  double *inv_ls = nullptr;    // [k][dp]        1 / ls (the query side multiplies; the training side X / ls is exact)
  double *ls = nullptr;        // [k][dp]        length scales (padded dims = 1)
  double *constv = nullptr;    // [k]
  double *kdiag = nullptr;     // [k]  kernel_.diag = 1 (+const) (+noise)
  double *alpha = nullptr;     // [k][Npad] (padded = 0)
  double *cv_jit = nullptr;    // [k]  the fit's alpha jitter: L_00^2 - kdiag (cross-validation variances, k_cv.hip)
  double *Wt = nullptr;        // [k][Npad][Npad]  Wt[p][j][i] = (L_p^-1)[i][j]  (upper triangular)
  double *Xtr = nullptr;       // [Npad][dp]  raw training rows (padded rows / dims = 0): the joint covariance (k_pcov.hip)
  std::vector<double> h_kdiag, h_noise;   // host copies [k] of kernel_.diag and of the White level (0 without one): k_design.hip

  // PCA / scaler
  double *comp = nullptr;      // [k][F]
  double *smean = nullptr;     // [F]
  double *sscale = nullptr;    // [F]
  double *cunexpl = nullptr;   // [F][F] (zeros if not given)

  // likelihood state (gpemu_likelihood_setup)
  bool lik_ready = false;
  double n_div = 1.0;
  int lik_chains = 1;          // data vectors the likelihood was set up for (one per chain of a multi-chain sampler)
  int64_t variant_B = 0;       // if > 0: pick the kernel variants as for a batch of this size (sampler with several chains)
  // the constants (G, g0, scal) depend on the data AND on n_div (the reference divides the truncation covariance by
  // the number of in-bounds rows of each call): one entry per n_div seen with the current data, so that a batch
  // size that comes back costs nothing.  G / g0 / scal below point into the current entry.
  struct LikEntry { double n_div; double *G, *g0, *scal, *W, *Q, *w0; };
  std::vector<LikEntry> lik_cache;
  std::vector<double> lik_host;        // y_exp | y_err | lo | hi | block starts | cov | sources the cache belongs to
  double *yexp = nullptr, *yerr = nullptr, *lo = nullptr, *hi = nullptr;  // [F],[F],[dp],[dp]
  int64_t nblk = 1;            // observable blocks of the (block-diagonal) covariance
  int *blk_start = nullptr;    // [nblk+1] first feature of each block
  int *blk_of = nullptr;       // [F]      block index of each feature
  double *G = nullptr;         // [nblk][k][k]   U_o^T A_o^-1 U_o
  double *g0 = nullptr;        // [nblk][k]      U_o^T A_o^-1 r0_o
  double *scal = nullptr;      // [nblk][2]      q0_o, logdet A_o
  // correlated data uncertainties (k_srccorr.hip): C_d = blockdiag_o(C_o) + sum_s b_s b_s^T
  double *ycov = nullptr;      // [F][F] within-observable data covariance C_o, or null: diag(y_err^2)
  double *srcs = nullptr;      // [n_src][F] fully correlated systematic sources b_s (this group's columns)
  int n_src = 0;               // S, 0 .. GPEMU_MAX_SOURCES
  double *W = nullptr;         // [nblk][k][S]   U_o^T A_o^-1 B_o
  double *Q = nullptr;         // [nblk][S][S]   B_o^T A_o^-1 B_o
  double *w0 = nullptr;        // [chains][nblk][S]  B_o^T A_o^-1 r0_o

  // workspace of the derivative calls (k_grad.hip): allocated by the first of them, null until then
  double *grad_ws = nullptr;
  double *grad_lik_ws = nullptr;   // the likelihood's per-(row, observable block) terms, grown with the number of blocks
  int64_t grad_lik_cap = 0;

  // exact-form (validation) scratch: per-workgroup Sigma, panel and residual
  double *exact_scratch = nullptr;
  int64_t exact_scratch_size = 0;

  // optional per-kernel timing (gpemu_model_profile): HIP event pairs around the two hot kernels
  bool profiling = false;
  std::vector<hipEvent_t> ev_pool;         // reusable events
  std::vector<std::pair<int, int>> ev_trmm, ev_kstar;  // indices into ev_pool (start, stop)
  size_t ev_next = 0;
  double prof_ms[2] = {0.0, 0.0};          // accumulated: [0] trmm_vsq, [1] kstar
  int64_t prof_n[2] = {0, 0};
  // device, [2]: proposals inside the prior box / proposals formed by the compacted half-steps of samplers over this
  // model (k_sampler.hip: propose_compact_kernel) since gpemu_model_profile was last called
  long long *live_cnt = nullptr;

  gpemu::Workspace ws;
};

namespace gpemu {
// A[f][g] + the data covariance's entry (likelihood setup, exact form): C_o where given (ycov, k_srccorr.hip), else
// diag(y_err^2).  A diagonal entry of C_o equal to y_err_f^2 is added as the default adds it, fma(y_err_f, y_err_f, v):
// cov = diag(y_err^2) gives the bits of the setup without cov.
__device__ inline double add_data_cov(double v, int f, int g, int64_t idx, const double *yerr, const double *ycov) {
  if (ycov && (f != g || ycov[idx] != yerr[f] * yerr[f])) return v + ycov[idx];
  return (f == g) ? fma(yerr[f], yerr[f], v) : v;
}

// optional fused stretch-move finish (accept / reject + chain record) for the walker of each proposal
struct AcceptArgs {
  int enabled = 0;
  double *X = nullptr;            // [W][dp] ensemble positions (updated in place)
  double *logp = nullptr;         // [W]
  const int *idx_s = nullptr;     // [ns] walker of proposal i
  const double *factors = nullptr;  // [ns] (d-1) log zz
  const double *logu = nullptr;   // [ns] log of the accept uniform
  long long *naccept = nullptr;   // [W]
  int *flags = nullptr;           // [1] NaN counter
  double *chain = nullptr;        // [W][d] row of this step, or null
  double *lpchain = nullptr;      // [W]
  // several chains stacked in one batch: row b of the launch is row first + b of the stacked list, which holds
  // chain_per rows per chain; 0 = one chain.  Selects the chain's data constants (g0, q0) in the likelihood.
  int chain_per = 0;
  int64_t first = 0;
  int dp = DPAD;                  // padded width of X and of the query rows (the models' dp)
  // parallel tempering (k_temper.hip): the rungs are chain_per-row chains that share data vector 0 (chain_data = 0)
  // and scale the accept test by their inverse temperature beta[(first + b) / chain_per]; null: untempered
  const double *beta = nullptr;
  int chain_data = 1;             // with chain_per != 0: the row's chain selects the data constants (g0, q0)
  // compacted half-step (k_sampler.hip: propose_compact_kernel): proposal b's query row, partial sums and new position
  // are those of column slot_of[b]; a negative slot is a proposal outside the prior box, which has none.  null: column b
  const int *slot_of = nullptr;
};

// stretch-move accept of a proposal (log-probability nlp) for a walker at oldlp, at inverse temperature beta.
// beta = 1 is the untempered test, bit for bit.  Otherwise the infinite cases are decided explicitly -- at beta = 0,
// 0 * (nlp - oldlp) would be NaN for either -- as every beta > 0 decides them: a proposal of non-finite
// log-probability is rejected, a walker at -inf (a start outside the open box) takes any finite proposal; else the
// log-likelihood difference is scaled by beta.
__host__ __device__ inline bool tempered_accept(double factor, double nlp, double oldlp, double logu, double beta) {
  if (beta == 1.0) return (factor + nlp - oldlp) > logu;
  if (!__builtin_isfinite(nlp)) return false;
  if (oldlp == -INFINITY) return true;
  return factor + beta * (nlp - oldlp) > logu;
}

// optional fused stretch-move proposal: kstar_kernel builds its query rows from the ensemble
// (q_i = c[rint_i] - (c[rint_i] - s_i) zz_i, emcee moves/stretch.py) instead of reading them
struct ProposeArgs {
  int enabled = 0;
  const double *X = nullptr;      // [W][dpad_of(d)]
  const int *idx_s = nullptr;     // [n] walker of proposal i (already offset to the evaluated slice)
  const double *zz = nullptr;     // [n]
  const int *partner = nullptr;   // [n] walker index of the complementary-set member drawn for proposal i
  double *factors = nullptr;      // [n] out: (d - 1) log zz
  int n = 0, d = 0;
  // enabled == 0 and raw != nullptr: the queries come as caller rows [n][d] (gpemu_gp_predict / predict_full); the
  // kernel pads them to [..][dpad_of(d)] on the fly and stores the padded rows once (what pad_queries_kernel used to do)
  const double *raw = nullptr;
};

// The sampler's compacted half-step: the first *n_live rows of the padded query buffer are the proposals inside the
// prior box, and the cross-kernel and the triangular GEMM serve only the ceil(*n_live / 64) column blocks that hold them
// (the count is known on the device alone: the grids stay those of the whole batch).  form: how the live blocks are
// dealt to the XCDs -- 0 the whole batch's schedule, 1 the whole batch's placement without the dead blocks, 2 by cost
// (k_predict.hip: build_trmm_schedule), -1 the measured choice per count
struct LiveCols {
  const int *n_live = nullptr;
  int form = -1;
};

int ensure_workspace(gpemu_model *m, int64_t B);
// base kernel of the kernel templates (fit, cross-kernel, covariance): 0 RBF (and Matern nu = inf, skl
// kernels.py:1722-1723), 1 / 2 / 3 Matern 0.5 / 1.5 / 2.5 (closed forms: matern_dev.h, base_from_r2), 4 Matern of any
// other nu (matern_dev.h; in the cross-kernel its constants behind etab's table)
static inline int base_kind(int kernel_kind, double nu) {
  if (kernel_kind == GPEMU_KERNEL_RBF) return 0;
  if (nu == 0.5) return 1;
  if (nu == 1.5) return 2;
  if (nu == 2.5) return 3;
  if (nu == INFINITY) return 0;
  return 4;
}
static inline int kstar_kind(const gpemu_model *m) { return base_kind(m->kernel_kind, m->nu); }
// the runtime base kind as a template argument: returns fn(std::integral_constant<int, K>{}) for K = kind in 0 .. 4
template <class Fn>
static inline int with_base_kind(int kind, Fn &&fn) {
  switch (kind) {
    case 0: return fn(std::integral_constant<int, 0>{});
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    default: set_error("unknown base kernel %d", kind); return GPEMU_ERR_STATE;
  }
}
// two models whose cross-kernels can share one launch: the same base kernel (and, for kind 4, the same nu)
static inline bool kstar_same_kernel(const gpemu_model *a, const gpemu_model *b) {
  return kstar_kind(a) == kstar_kind(b) && (kstar_kind(a) != 4 || a->nu == b->nu);
}

// kernels (launchers; all asynchronous on `st`)
// dXq_padded is read, or -- with pa->enabled -- written (rows [0, round_up(B, 128))) by the kernel
int launch_kstar(gpemu_model *m, int64_t B, double *dXq_padded, hipStream_t st, const ProposeArgs *pa = nullptr,
                 const LiveCols *lv = nullptr);
int launch_trmm_vsq(gpemu_model *m, int64_t B, hipStream_t st, const LiveCols *lv = nullptr);
// builds (once per model, shape and form) the tables the two launches above pick from with `lv` for batches of B columns:
// the sampler calls it when it is created, so that no run allocates or copies them.  GPEMU_ERR_UNSUPPORTED: a shape the
// tables cannot describe -- the caller evaluates every proposal instead
int prepare_live_cols(gpemu_model *m, int64_t B, int form, hipStream_t st);
int small_trmm_xcd_of(const gpemu_model *m, int64_t B, int p, int64_t col);
int trmm_xcd_of(const gpemu_model *m, int64_t B, int p, int64_t col);   // XCD that reads K_*^T rows (p, col) in launch_trmm_vsq(m, B); -1: any
int launch_trmm_vsq_small(gpemu_model *m, int64_t B, hipStream_t st);   // B <= 128; GPEMU_ERR_UNSUPPORTED if the shape does not fit
int launch_reduce_mean_var(gpemu_model *m, int64_t B, double *dmean, double *dvar, hipStream_t st);
// The switches that choose among the log-posterior's launch forms (the same bits; tests compare them).  Their only
// reader, read_launch_switches, runs once per public call: never cached, tests change them between calls.
struct LaunchSwitches {
  bool halfstep;                  // not GPEMU_NO_HALFSTEP and not GPEMU_NO_GROUP_MERGE: small emulators' one-launch form
  bool group_merge;               // not GPEMU_NO_GROUP_MERGE: one launch per stage for all groups
  bool loglik_tasks;              // not GPEMU_NO_LOGLIK_TASKS: observable blocks on different waves
  int halfstep_min_pairs;         // GPEMU_HALFSTEP_MIN_PAIRS, default 64
  int64_t loglik_tasks_max_rows;  // GPEMU_LOGLIK_TASKS_MAX_ROWS, default 256
  bool compact;                   // not GPEMU_NO_COMPACT: the sampler's half-step evaluates only the proposals inside the prior box
  int compact_form;               // GPEMU_COMPACT_FORM (measurements: LiveCols::form for every count), default -1
};
LaunchSwitches read_launch_switches();
// log-posterior of B padded query rows summed over ng groups: the one place that chooses the launches (gpemu_api.hip)
int logpost_eval(gpemu_model *const *ms, int ng, int64_t B, double *dXq, double *dout, hipStream_t st,
                 const LaunchSwitches &sw, const AcceptArgs *aa, const ProposeArgs *pa, const LiveCols *lv = nullptr);
int launch_loglik_lowrank(gpemu_model *m, int64_t B, const double *dXq_padded, double *dout,
                          int accumulate, hipStream_t st, const AcceptArgs *aa);
// several emulation groups, one launch per stage instead of one per group and stage (k_predict.hip, k_trmm_small.hip,
// k_loglik.hip): the same arithmetic as the per-group launches
int launch_kstar_groups(gpemu_model *const *ms, int ng, int64_t B, double *dXq_padded, hipStream_t st, const ProposeArgs *pa);
int prepare_trmm_vsq_small_groups(gpemu_model *const *ms, int ng, int64_t B, hipStream_t st);   // the schedules only
int launch_trmm_vsq_small_groups(gpemu_model *const *ms, int ng, int64_t B, hipStream_t st);
int launch_loglik_groups(gpemu_model *const *ms, int ng, int64_t B, const double *dXq_padded, double *dout, int accumulate,
                         hipStream_t st, const AcceptArgs *aa);
// the likelihood with the observable blocks on different waves (k_loglik.hip), where loglik_tasks_fit
bool loglik_tasks_fit(gpemu_model *const *ms, int ng, int64_t B, const AcceptArgs *aa, const LaunchSwitches &sw);
int launch_loglik_tasks(gpemu_model *const *ms, int ng, int64_t B, const double *dXq_padded, double *dout, int accumulate,
                        hipStream_t st, const AcceptArgs *aa);
// the fully correlated sources' term (k_srccorr.hip), after the likelihood stage of all ng groups (which wrote their
// block-diagonal sum to dout and left the accept to this launch): adds the Woodbury correction, finishes the stretch move
int launch_source_correction(gpemu_model *const *ms, int ng, int64_t B, const double *dXq_padded, double *dout,
                             hipStream_t st, const AcceptArgs *aa);
// small emulators (N <= 256 design points, k_halfstep.hip): cross-kernel + triangular GEMM of all groups in one launch,
// then the likelihood launch; the bits of the general path.  Launch only where halfstep_fits
bool halfstep_fits(gpemu_model *const *ms, int ng, int64_t B, const LaunchSwitches &sw);
int launch_halfstep_small(gpemu_model *const *ms, int ng, int64_t B, double *dXq_padded, hipStream_t st, const ProposeArgs *pa);
// fit-side building blocks (k_fit.hip): in-place blocked Cholesky of an Np x Np matrix (Np multiple of 64) with the
// inverted diagonal blocks in Dinv [Np/64][64][64], and W = L^-1 from it (T: Np x Np scratch)
// Optional look-ahead of the blocked Cholesky: a second (lower-priority) stream that applies a panel's update to the
// columns beyond the next panel while the next panel is factored on the caller's stream (k_fit.hip).
struct CholOverlap {
  hipStream_t side = nullptr;
  hipEvent_t panel_done = nullptr, rest_done = nullptr;
  int *flags = nullptr;      // device, 20 ints per problem: enables the one-launch-per-panel kernel (k_fit.hip)
};
int device_cholesky_blocked(double *A, int64_t Np, double *Dinv, int *dinfo, hipStream_t st, int nb = 1,
                            const CholOverlap *ov = nullptr);
int device_trtri_blocked(const double *L, int64_t Np, const double *Dinv, double *W, double *T, hipStream_t st, int nb = 1,
                         bool zero_upper = true);
int device_invert_factor_to_Wt(const double *dL, int64_t N, double *Wt, int64_t Npad, double *A, double *Dinv,
                               double *W, double *T, hipStream_t st);
// cross-validation at the fitted theta (k_cv.hip): per-(PC, fold) means / variances into dmean / dvar [N][k], then the
// observable-space back-projection (either output may be null)
int cross_validate(gpemu_model *m, int n_folds, const int *didx, const int *dfoff, const std::vector<int> &hfoff,
                   const std::vector<int> &hr0, const double *dy, double *dmean, double *dvar, int64_t max_chunk);
int launch_cv_backproject(gpemu_model *m, const double *dmean, const double *dvar, double *dcv, double *dvo);
// joint predictive covariance (k_pcov.hip): dcov [k][M1][M2] of the query rows dX1 [M1][d] and dX2 [M2][d] (null: the
// symmetric form on dX1, noise on the diagonal); workspace_bytes <= 0: sized from free device memory.  Synchronises st.
int predict_cov(gpemu_model *m, int64_t M1, const double *dX1, int64_t M2, const double *dX2, int64_t workspace_bytes,
                double *dcov, hipStream_t st);
// draws dout [k][M][n] = mean + chol(C_p + tau_p I) z_p from the symmetric dcov [k][M][M], dmean [M][k], dz [k][M][n];
// tau_out[k] on the host.  Returns p + 1 for the first PC whose jitter ladder is exhausted.
int sample_from_cov(gpemu_model *m, int64_t M, int64_t n, const double *dcov, const double *dmean, const double *dz,
                    double *dout, double *tau_out, hipStream_t st);
// the derivative path (k_grad.hip) for the HMC sampler (k_hmc.hip): what it declines (GPEMU_ERR_UNSUPPORTED: Matern 0.5
// and general nu, n_src > 0, several data vectors), and lp [B], grad [B][d] of the unpadded rows dX [B][d] summed over
// ng groups the caller has checked, asynchronous on st
int grad_lik_supported(const gpemu_model *m, const char *what);
int logpost_grad_eval(gpemu_model *const *ms, int ng, int64_t B, const double *dX, double *dlp, double *dgrad,
                      hipStream_t st);
// profiling helpers: record an event on `st` and return its pool index (-1 when profiling is off)
int prof_mark(gpemu_model *m, hipStream_t st);
void prof_pair(gpemu_model *m, int which, int e0, int e1);
}  // namespace gpemu

#include "devmem.h"   // who owns device memory: DevScope, dev_reserve, dev_alloc / dev_free
