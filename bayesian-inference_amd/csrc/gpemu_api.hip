// C ABI of libgpemu.so (see include/gpemu.h).  Host-side glue: argument checks, device memory
// ownership (devmem.h), launch sequencing.  The arithmetic is in the k_*.hip kernels, with one
// exception: trunc_pack_kernel, the operand packing of gpemu_truncation_cov, sits next to its caller.
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <mutex>
#include <set>

#include "internal.h"
#include "kstar_host.h"
#include "matern_dev.h"
#include "gemm.h"
#include "linalg_dev.h"

namespace gpemu {

static thread_local char g_err[512] = "";

// the path counters of every family (internal.h: PathFamily), a row each
constexpr int PATH_FAMILY_SIZE[PATH_FAMILIES] = {GPEMU_PATH_COUNT, GPEMU_FIT_PATH_COUNT, GPEMU_WIDE_PATH_COUNT,
                                                 GPEMU_SRC_PATH_COUNT, GPEMU_GRAD_PATH_COUNT, GPEMU_POSTPRED_PATH_COUNT,
                                                 GPEMU_HMC_PATH_COUNT, GPEMU_DIAG_PATH_COUNT, GPEMU_SOBOL_PATH_COUNT,
                                                 GPEMU_MARGINAL_PATH_COUNT, GPEMU_DESIGN_PATH_COUNT,
                                                 GPEMU_KDE2D_PATH_COUNT, GPEMU_LOO_PATH_COUNT, GPEMU_KNN_PATH_COUNT,
                                                 GPEMU_PAIRLSE_PATH_COUNT, GPEMU_REWEIGHT_PATH_COUNT,
                                                 GPEMU_WSUMMARY_PATH_COUNT, GPEMU_SOBOL_PAIRS_PATH_COUNT};
constexpr int PATH_ROW = 32;
static_assert(GPEMU_PATH_COUNT <= PATH_ROW && GPEMU_FIT_PATH_COUNT <= PATH_ROW && GPEMU_WIDE_PATH_COUNT <= PATH_ROW &&
              GPEMU_SRC_PATH_COUNT <= PATH_ROW && GPEMU_GRAD_PATH_COUNT <= PATH_ROW && GPEMU_POSTPRED_PATH_COUNT <= PATH_ROW &&
              GPEMU_HMC_PATH_COUNT <= PATH_ROW && GPEMU_DIAG_PATH_COUNT <= PATH_ROW && GPEMU_SOBOL_PATH_COUNT <= PATH_ROW &&
              GPEMU_MARGINAL_PATH_COUNT <= PATH_ROW && GPEMU_DESIGN_PATH_COUNT <= PATH_ROW &&
              GPEMU_KDE2D_PATH_COUNT <= PATH_ROW && GPEMU_LOO_PATH_COUNT <= PATH_ROW && GPEMU_KNN_PATH_COUNT <= PATH_ROW &&
              GPEMU_PAIRLSE_PATH_COUNT <= PATH_ROW && GPEMU_REWEIGHT_PATH_COUNT <= PATH_ROW &&
              GPEMU_WSUMMARY_PATH_COUNT <= PATH_ROW && GPEMU_SOBOL_PAIRS_PATH_COUNT <= PATH_ROW,
              "a family outgrew its row");
static std::atomic<int64_t> g_path_counts[PATH_FAMILIES][PATH_ROW];

void count_path(PathFamily family, int path) {
  if (path >= 0 && path < PATH_FAMILY_SIZE[family]) g_path_counts[family][path].fetch_add(1, std::memory_order_relaxed);
}

int read_path_counts(PathFamily family, int64_t *out, int64_t n) {
  GP_ARG(out && n >= 0, "out, n");
  const int size = PATH_FAMILY_SIZE[family];
  for (int64_t i = 0; i < n && i < size; ++i) out[i] = g_path_counts[family][i].load(std::memory_order_relaxed);
  return size;
}

// the one ledger of device resources (devledger.h), fed by devmem.h from every translation unit
DevLedger &dev_ledger() {
  static DevLedger ledger;
  return ledger;
}

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int allow_dynamic_lds(const void *fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void *, int>> allowed;   // (function, device) pairs whose attribute is set
  int dev = 0;
  GP_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (allowed.count({fn, dev})) return GPEMU_OK;
  GP_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  allowed.insert({fn, dev});
  return GPEMU_OK;
}

int launch_lik_setup(gpemu_model *m, const std::vector<int> &hstart, double *dA, double *dPT, double *dZ, int *dinfo,
                     hipStream_t st);
int launch_predict_full(gpemu_model *m, int64_t B, double n_div, double *dcv, double *dcov, hipStream_t st,
                        const double *dmean, const double *dvar);
int launch_loglik_exact(gpemu_model *m, int64_t B, const double *dXq, double *dout, hipStream_t st);


static void free_lik_entry(gpemu_model::LikEntry &en) {
  dev_free(en.G); dev_free(en.g0); dev_free(en.scal);
  dev_free(en.W); dev_free(en.Q); dev_free(en.w0);
}

static void free_workspace(Workspace &w) {
  dev_free(w.Xq); dev_free(w.KS); dev_free(w.mean_part); dev_free(w.mean_part2); dev_free(w.vsq_part);
  dev_free(w.mean); dev_free(w.var); dev_free(w.logp);
  w = Workspace();
}

int ensure_workspace(gpemu_model *m, int64_t B) {
  Workspace &w = m->ws;
  int64_t need = round_up(B < 1 ? 1 : B, TILE);
  if (need <= w.Bcap) return GPEMU_OK;
  GP_HIP(hipStreamSynchronize(m->stream));
  free_workspace(w);
  const int64_t k = m->k;
  GP_TRY(dev_alloc(&w.Xq, need * m->dp));
  GP_TRY(dev_alloc(&w.KS, k * m->Npad * need));
  GP_TRY(dev_alloc(&w.mean_part, k * (m->Npad / 32) * need));   // sized for the 32-row small-batch form
  GP_TRY(dev_alloc(&w.mean_part2, k * (m->Npad / 32) * need));
  GP_TRY(dev_alloc(&w.vsq_part, k * (m->Npad / 32) * need));   // sized for the 32-row small-batch form
  GP_TRY(dev_alloc(&w.mean, need * k));
  GP_TRY(dev_alloc(&w.var, need * k));
  GP_TRY(dev_alloc(&w.logp, need));
  GP_HIP(hipMemsetAsync(w.KS, 0, sizeof(double) * (size_t)(k * m->Npad * need), m->stream));
  GP_HIP(hipMemsetAsync(w.Xq, 0, sizeof(double) * (size_t)(need * m->dp), m->stream));
  GP_HIP(hipMemsetAsync(w.vsq_part, 0, sizeof(double) * (size_t)(k * (m->Npad / 32) * need), m->stream));
  // the caller's launches may go to ANOTHER stream (a sampler over several groups runs every group on the first
  // group's stream): the zero fill must have landed before anything writes the new buffers (found by the shipped
  // three-group golden G7: the fill of groups 2 and 3 raced with their first evaluation and wiped partial sums)
  GP_HIP(hipStreamSynchronize(m->stream));
  w.Bcap = need;
  return GPEMU_OK;
}

// ---- optional per-kernel timing ---------------------------------------------------------------
static void prof_drain(gpemu_model *m) {
  // all recorded events must have completed (callers synchronise the stream first)
  for (int which = 0; which < 2; ++which) {
    auto &v = which == 0 ? m->ev_trmm : m->ev_kstar;
    for (auto &pr : v) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, m->ev_pool[pr.first], m->ev_pool[pr.second]) == hipSuccess) {
        m->prof_ms[which] += ms;
        m->prof_n[which] += 1;
      }
    }
    v.clear();
  }
  m->ev_next = 0;
}

int prof_mark(gpemu_model *m, hipStream_t st) {
  if (!m->profiling) return -1;
  if (m->ev_next >= 8192) {  // bounded pool: fold what we have into the totals and reuse
    (void)hipStreamSynchronize(st);
    prof_drain(m);
  }
  if (m->ev_next >= m->ev_pool.size()) {
    hipEvent_t e;
    if (event_create(&e) != hipSuccess) return -1;
    m->ev_pool.push_back(e);
  }
  int idx = (int)m->ev_next++;
  if (hipEventRecord(m->ev_pool[idx], st) != hipSuccess) return -1;
  return idx;
}

void prof_pair(gpemu_model *m, int which, int e0, int e1) {
  if (!m->profiling || e0 < 0 || e1 < 0) return;
  (which == 0 ? m->ev_trmm : m->ev_kstar).emplace_back(e0, e1);
}

int device_ready(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_error("no HIP device available: libgpemu has no CPU implementation");
    return GPEMU_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= n) {
    set_error("device %d out of range (have %d)", device, n);
    return GPEMU_ERR_ARG;
  }
  GP_HIP(hipSetDevice(device));
  return GPEMU_OK;
}

LaunchSwitches read_launch_switches() {
  LaunchSwitches sw;
  sw.group_merge = getenv("GPEMU_NO_GROUP_MERGE") == nullptr;
  sw.halfstep = sw.group_merge && getenv("GPEMU_NO_HALFSTEP") == nullptr;   // "stage by stage, group by group" includes it
  sw.loglik_tasks = getenv("GPEMU_NO_LOGLIK_TASKS") == nullptr;
  const char *e = getenv("GPEMU_HALFSTEP_MIN_PAIRS");
  sw.halfstep_min_pairs = e ? atoi(e) : 64;
  e = getenv("GPEMU_LOGLIK_TASKS_MAX_ROWS");
  sw.loglik_tasks_max_rows = e ? atoll(e) : 256;
  sw.compact = getenv("GPEMU_NO_COMPACT") == nullptr;
  e = getenv("GPEMU_COMPACT_FORM");
  sw.compact_form = e ? atoi(e) : -1;
  return sw;
}

// Eligible for one launch per stage for all groups: at most 128 columns (the small-batch GEMM), at most 32 PCs per
// group, one base kernel, parameter count and device.  A sampler over the reference's shipped three groups (5 / 11 / 25
// PCs, ~150 design points, 200 walkers) spends its half-step in nine ~6 us launches otherwise; the kernels' work per
// group is the per-group launches' (same device functions, the groups' terms added in the same order): the same bits.
static bool groups_fit(gpemu_model *const *ms, int ng, int64_t B) {
  if (ng < 2 || ng > 8 || B < 1 || B > 128) return false;
  for (int g = 0; g < ng; ++g) {
    const gpemu_model *m = ms[g];
    const int64_t Bv = m->variant_B > 0 ? m->variant_B : B;
    if (Bv > 128 || m->k > 32 || m->d != ms[0]->d || !kstar_same_kernel(m, ms[0]) || m->ksteps != ms[0]->ksteps ||
        m->device != ms[0]->device || m->profiling)
      return false;
  }
  return true;
}

// The query rows are in the padded [rows >= round_up(B,128)][dp] layout (the sampler writes its proposals in it), or
// `pa` builds them there.  In order of preference: (1) cross-kernel and GEMM of every group in one launch (small
// emulators, k_halfstep.hip); (2) for several groups, one launch per stage; (3) group by group, the groups after the
// first adding to dout.  Stacked chains take neither (1) nor (2).  Every form gives the same bits.
// what the groups' setups must agree on before anything is evaluated; the host-array entries ask it before they stage
// their rows, so that a call that is declined has allocated nothing
static int logpost_groups_ready(gpemu_model *const *ms, int ng) {
  for (int g = 0; g < ng; ++g)
    if (!ms[g]->lik_ready) { set_error("gpemu_likelihood_setup has not been called"); return GPEMU_ERR_STATE; }
  for (int g = 1; g < ng; ++g)
    if (ms[g]->n_src != ms[0]->n_src) {
      set_error("groups set up with different numbers of correlated sources (%d and %d)", ms[0]->n_src, ms[g]->n_src);
      return GPEMU_ERR_STATE;
    }
  return GPEMU_OK;
}
// ... and a single model's mode
static int logpost_mode_ready(const gpemu_model *m, int mode) {
  GP_ARG(mode == GPEMU_LOGPOST_LOWRANK || mode == GPEMU_LOGPOST_EXACT, "mode");
  if (!m->lik_ready) { set_error("gpemu_likelihood_setup has not been called"); return GPEMU_ERR_STATE; }
  if (mode == GPEMU_LOGPOST_EXACT && m->n_src > 0) {
    set_error("GPEMU_LOGPOST_EXACT does not support correlated sources (n_src = %d): use GPEMU_LOGPOST_LOWRANK", m->n_src);
    return GPEMU_ERR_UNSUPPORTED;
  }
  return GPEMU_OK;
}

int logpost_eval(gpemu_model *const *ms, int ng, int64_t B, double *dXq, double *dout, hipStream_t st,
                 const LaunchSwitches &sw, const AcceptArgs *aa, const ProposeArgs *pa, const LiveCols *lv) {
  if (lv && (ng != 1 || ms[0]->n_src != 0 || (aa && aa->chain_per != 0) || halfstep_fits(ms, 1, B, sw) ||
             loglik_tasks_fit(ms, 1, B, aa, sw))) {
    set_error("logpost_eval: compacted columns outside the general path of one group");   // (the caller's eligibility test)
    return GPEMU_ERR_STATE;
  }
  GP_TRY(logpost_groups_ready(ms, ng));
  // correlated sources (k_srccorr.hip): one set of sources for all groups, whose term follows the likelihood stage
  const int S = ms[0]->n_src;
  // Stacked chains: a row's chain selects its data vector in a group whose CURRENT setup carries one per chain; a group
  // set up with one vector serves every chain with it (by_chain_of).  A setup with fewer vectors than the rows have chains
  // -- changed under a live sampler -- is refused before anything is launched: g0 / scal / w0 end at its last vector.
  const bool by_chain = aa && aa->chain_per != 0 && aa->chain_data != 0;
  if (by_chain) {
    const int64_t last = (aa->first + B - 1) / aa->chain_per;
    for (int g = 0; g < ng; ++g) {
      if (ms[g]->lik_chains != 1 && ms[g]->lik_chains <= last) {
        set_error("group %d is set up with %d data vectors, the sampler's rows reach chain %lld: the likelihood setup "
                  "changed under a stacked sampler", g, ms[g]->lik_chains, (long long)last);
        return GPEMU_ERR_STATE;
      }
      if (S > 0 && ms[g]->lik_chains != ms[0]->lik_chains) {
        set_error("groups with correlated sources set up with different numbers of data vectors (%d and %d)",
                  ms[0]->lik_chains, ms[g]->lik_chains);
        return GPEMU_ERR_STATE;
      }
    }
  }
  auto by_chain_of = [&](const gpemu_model *m, const AcceptArgs *a) {
    AcceptArgs out = *a;
    if (by_chain && m->lik_chains == 1) out.chain_data = 0;
    return out;
  };
  for (int g = 0; g < ng; ++g) GP_TRY(ensure_workspace(ms[g], B));
  // the likelihood stage: observable blocks on different waves where that applies, else one launch for the groups
  auto loglik = [&](gpemu_model *const *gs, int n, int accumulate, const AcceptArgs *a) {
    if (loglik_tasks_fit(gs, n, B, a, sw)) return launch_loglik_tasks(gs, n, B, dXq, dout, accumulate, st, a);
    if (n == 1) return launch_loglik_lowrank(gs[0], B, dXq, dout, accumulate, st, a);
    return launch_loglik_groups(gs, n, B, dXq, dout, accumulate, st, a);
  };
  AcceptArgs chain_only;                 // groups before the last: no accept, but the rows' chains (data constants)
  if (aa) { chain_only.chain_per = aa->chain_per; chain_only.first = aa->first; chain_only.chain_data = aa->chain_data; }
  // with sources the likelihood stage leaves the accept to the sources' launch
  const AcceptArgs *aa_lik = (S > 0 && aa) ? &chain_only : aa;
  auto finish = [&]() {
    if (S == 0) return (int)GPEMU_OK;
    if (!by_chain) return launch_source_correction(ms, ng, B, dXq, dout, st, aa);
    const AcceptArgs a0 = by_chain_of(ms[0], aa);
    return launch_source_correction(ms, ng, B, dXq, dout, st, &a0);
  };
  const bool one_chain = !(aa && aa->chain_per != 0);
  if (one_chain && halfstep_fits(ms, ng, B, sw)) {
    GP_TRY(launch_halfstep_small(ms, ng, B, dXq, st, pa));
    GP_TRY(loglik(ms, ng, 0, aa_lik));
    return finish();
  }
  if (one_chain && sw.group_merge && groups_fit(ms, ng, B)) {
    // (the GEMM's schedules first: the one step that can still decline, before anything is launched)
    const int rc = prepare_trmm_vsq_small_groups(ms, ng, B, st);
    if (rc != GPEMU_ERR_UNSUPPORTED) {
      GP_TRY(rc);
      GP_TRY(launch_kstar_groups(ms, ng, B, dXq, st, pa));
      GP_TRY(launch_trmm_vsq_small_groups(ms, ng, B, st));
      GP_TRY(loglik(ms, ng, 0, aa_lik));
      return finish();
    }
  }
  for (int g = 0; g < ng; ++g) {
    gpemu_model *const *one = ms + g;
    const ProposeArgs *pg = g == 0 ? pa : nullptr;
    if (one_chain && halfstep_fits(one, 1, B, sw)) {
      GP_TRY(launch_halfstep_small(one, 1, B, dXq, st, pg));
    } else {
      path_count(GPEMU_PATH_HALFSTEP_GENERAL);
      GP_TRY(launch_kstar(ms[g], B, dXq, st, pg, lv));
      GP_TRY(launch_trmm_vsq(ms[g], B, st, lv));
    }
    const AcceptArgs *ag = g + 1 == ng ? aa_lik : (aa ? &chain_only : nullptr);
    AcceptArgs own;
    if (by_chain) { own = by_chain_of(ms[g], ag); ag = &own; }
    GP_TRY(loglik(one, 1, g > 0 ? 1 : 0, ag));
  }
  return finish();
}
}  // namespace gpemu

using namespace gpemu;

extern "C" {

const char *gpemu_version(void) { return "gpemu 0.1 (gfx950)"; }
const char *gpemu_last_error(void) { return g_err; }

int gpemu_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_LOGPOST, out, n); }
int gpemu_fit_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_FIT, out, n); }
int gpemu_wide_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_WIDE, out, n); }
int gpemu_src_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_SRC, out, n); }
int gpemu_grad_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_GRAD, out, n); }

int gpemu_devmem_stats(int64_t *out, int64_t n) {
  GP_ARG(out && n >= 0, "out, n");
  const DevLedger::Stats s = dev_ledger().stats();
  const int64_t v[GPEMU_DEVMEM_STAT_COUNT] = {s.live_blocks, s.live_bytes, s.allocs, s.frees, s.live_streams, s.live_events};
  for (int64_t i = 0; i < n && i < GPEMU_DEVMEM_STAT_COUNT; ++i) out[i] = v[i];
  return GPEMU_DEVMEM_STAT_COUNT;
}

int gpemu_devmem_refuse_nth(int64_t nth, int64_t *still_armed) {
  GP_ARG(nth >= 0, "nth >= 0");
  const bool was = dev_ledger().arm(nth);
  if (still_armed) *still_armed = was ? 1 : 0;
  return GPEMU_OK;
}

int gpemu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int gpemu_device_name(int device, char *buf, int64_t buflen) {
  GP_TRY(device_ready(device));
  GP_ARG(buf && buflen > 0, "buf");
  hipDeviceProp_t prop;
  GP_HIP(hipGetDeviceProperties(&prop, device));
  snprintf(buf, (size_t)buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return GPEMU_OK;
}

int gpemu_device_bus_id(int device, char *buf, int64_t buflen) {
  GP_TRY(device_ready(device));
  GP_ARG(buf && buflen >= 16, "buf");
  GP_HIP(hipDeviceGetPCIBusId(buf, (int)buflen, device));
  return GPEMU_OK;
}

int gpemu_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes) {
  GP_TRY(device_ready(device));
  GP_ARG(free_bytes && total_bytes, "null pointer");
  size_t f = 0, t = 0;
  GP_HIP(hipMemGetInfo(&f, &t));
  *free_bytes = (int64_t)f;
  *total_bytes = (int64_t)t;
  return GPEMU_OK;
}

// the device state of a new model, whose dimensions are set: gpemu_model_create destroys `m` if this fails
static int model_fill(gpemu_model *m, const double *X_train, const double *ls, const double *constv, const double *noise,
                      const double *alpha, const double *L, const double *components, const double *scaler_mean,
                      const double *scaler_scale, const double *cov_unexplained) {
  const int64_t N = m->N, d = m->d, F = m->F, k = m->k, Np = m->Npad;
  const int has_const = m->has_const, has_noise = m->has_noise;
  const double nu = m->nu;
  if (stream_create(&m->stream, hipStreamNonBlocking) != hipSuccess) {
    set_error("hipStreamCreate failed");
    return GPEMU_ERR_HIP;
  }
  hipStream_t st = m->stream;
  DevScope sc(st);

  // host staging of the small padded arrays; `direct`: the kernels whose value is not flat at r = 0 (Matern 0.5, general
  // nu < 1) recompute the distance of near-coincident pairs from the coordinates (predict_dev.h: KstarDirect)
  const int kkind = kstar_kind(m);
  const bool direct = kkind == 1 || (kkind == 4 && nu < 1.0);
  const int dp = m->dp;
  std::vector<double> hXs(direct ? (size_t)(k * Np * dp) : 0, 0.0), hls((size_t)(k * dp), 1.0),
      hc((size_t)k, 0.0), hkd((size_t)k, 1.0), hal((size_t)(k * Np), 0.0), hjit((size_t)k, 0.0);
  for (int64_t p = 0; p < k; ++p) {
    for (int64_t dd = 0; dd < d; ++dd) {
      double l = ls[p * d + dd];
      if (!(l > 0.0)) { set_error("length scale must be positive"); return GPEMU_ERR_ARG; }
      hls[p * dp + dd] = l;
    }
    if (direct)
      for (int64_t j = 0; j < N; ++j)
        for (int64_t dd = 0; dd < d; ++dd)
          hXs[(p * Np + j) * dp + dd] = X_train[j * d + dd] / ls[p * d + dd];  // skl: X / length_scale
    if (has_const) { hc[p] = constv[p]; hkd[p] += constv[p]; }
    if (has_noise) hkd[p] += noise[p];
    for (int64_t j = 0; j < N; ++j) hal[p * Np + j] = alpha[p * N + j];
    // the fit's alpha jitter (skl _gpr.py:346-348: K + alpha I = L L^T): K_00 - kernel_.diag, K_00 = L_00^2
    hjit[p] = std::fma(L[p * N * N], L[p * N * N], -hkd[p]);
  }
  m->h_kdiag = hkd;
  m->h_noise.assign((size_t)k, 0.0);
  if (has_noise) m->h_noise.assign(noise, noise + k);
  double *dL = nullptr;
  GP_TRY(dev_alloc(&m->ls, k * dp));
  GP_TRY(dev_alloc(&m->constv, k));
  GP_TRY(dev_alloc(&m->kdiag, k));
  GP_TRY(dev_alloc(&m->alpha, k * Np));
  GP_TRY(dev_alloc(&m->cv_jit, k));
  GP_TRY(dev_alloc(&m->Wt, k * Np * Np));
  GP_TRY(dev_alloc(&m->Xtr, Np * dp));
  GP_TRY(dev_alloc(&m->comp, k * F));
  GP_TRY(dev_alloc(&m->smean, F));
  GP_TRY(dev_alloc(&m->sscale, F));
  GP_TRY(dev_alloc(&m->cunexpl, F * F));
  GP_TRY(dev_alloc(&m->live_cnt, 2));
  GP_HIP(hipMemsetAsync(m->live_cnt, 0, sizeof(long long) * 2, st));
  GP_TRY(sc.alloc(&dL, k * N * N));
  GP_TRY(upload(m->ls, hls.data(), k * dp, st));
  {
    std::vector<double> hX((size_t)(Np * dp), 0.0);
    for (int64_t j = 0; j < N; ++j)
      for (int64_t dd = 0; dd < d; ++dd) hX[(size_t)(j * dp + dd)] = X_train[j * d + dd];
    GP_TRY(upload(m->Xtr, hX.data(), Np * dp, st));
    if (hipStreamSynchronize(st) != hipSuccess) {   // hX goes out of scope
      set_error("model_create: upload failed");
      return GPEMU_ERR_HIP;
    }
  }
  {
    // the cross-kernel's operands for the matrix cores (kstar_host.h)
    KstarHost kh;
    build_kstar_operands(N, Np, d, k, kkind, X_train, ls, alpha, kh);
    if (kkind == 4) {   // the constants of nu behind the exponential's table (predict_dev.h: kstar_matern_nu)
      const MaternNu mn = matern_nu_constants(nu);
      const size_t n0 = kh.tab.size(), nw = (sizeof(MaternNu) + sizeof(double) - 1) / sizeof(double);
      kh.tab.resize(n0 + nw, 0.0);
      std::memcpy(kh.tab.data() + n0, &mn, sizeof(MaternNu));
    }
    m->ksteps = kh.ksteps;
    GP_TRY(dev_alloc(&m->Xa, (int64_t)kh.Xa.size()));
    GP_TRY(dev_alloc(&m->alf, (int64_t)kh.alf.size()));
    GP_TRY(dev_alloc(&m->qsc, (int64_t)kh.qsc.size()));
    GP_TRY(dev_alloc(&m->qof, (int64_t)kh.qof.size()));
    GP_TRY(dev_alloc(&m->etab, (int64_t)kh.tab.size()));
    GP_TRY(upload(m->Xa, kh.Xa.data(), (int64_t)kh.Xa.size(), st));
    GP_TRY(upload(m->alf, kh.alf.data(), (int64_t)kh.alf.size(), st));
    GP_TRY(upload(m->qsc, kh.qsc.data(), (int64_t)kh.qsc.size(), st));
    GP_TRY(upload(m->qof, kh.qof.data(), (int64_t)kh.qof.size(), st));
    GP_TRY(upload(m->etab, kh.tab.data(), (int64_t)kh.tab.size(), st));
    std::vector<double> hinv(hls.size());
    if (direct) {
      for (size_t i = 0; i < hls.size(); ++i) hinv[i] = 1.0 / hls[i];
      GP_TRY(dev_alloc(&m->Xs, k * Np * dp));
      GP_TRY(dev_alloc(&m->inv_ls, k * dp));
      GP_TRY(upload(m->Xs, hXs.data(), k * Np * dp, st));
      GP_TRY(upload(m->inv_ls, hinv.data(), k * dp, st));
    }
    if (hipStreamSynchronize(st) != hipSuccess) {   // the staging vectors go out of scope
      set_error("model_create: upload failed");
      return GPEMU_ERR_HIP;
    }
  }
  GP_TRY(upload(m->constv, hc.data(), k, st));
  GP_TRY(upload(m->kdiag, hkd.data(), k, st));
  GP_TRY(upload(m->alpha, hal.data(), k * Np, st));
  GP_TRY(upload(m->cv_jit, hjit.data(), k, st));
  GP_TRY(upload(m->comp, components, k * F, st));
  GP_TRY(upload(m->smean, scaler_mean, F, st));
  GP_TRY(upload(m->sscale, scaler_scale, F, st));
  if (cov_unexplained) {
    GP_TRY(upload(m->cunexpl, cov_unexplained, F * F, st));
  } else if (hipMemsetAsync(m->cunexpl, 0, sizeof(double) * (size_t)(F * F), st) != hipSuccess) {
    set_error("hipMemsetAsync failed");
    return GPEMU_ERR_HIP;
  }
  GP_TRY(upload(dL, L, k * N * N, st));
  {
    // W_p = L_p^-1 by the blocked MFMA triangular inverse, written transposed into Wt[p]
    const int64_t N64 = round_up(N, 64);
    DevScope inv(st);
    double *sA = nullptr, *sD = nullptr, *sW = nullptr, *sT = nullptr;
    GP_TRY(inv.alloc(&sA, N64 * N64));
    GP_TRY(inv.alloc(&sD, N64 * 64));
    GP_TRY(inv.alloc(&sW, N64 * N64));
    GP_TRY(inv.alloc(&sT, N64 * N64));
    if (hipMemsetAsync(m->Wt, 0, sizeof(double) * (size_t)(k * Np * Np), st) != hipSuccess) {
      set_error("hipMemsetAsync failed");
      return GPEMU_ERR_HIP;
    }
    for (int64_t p = 0; p < k; ++p)
      GP_TRY(device_invert_factor_to_Wt(dL + p * N * N, N, m->Wt + p * Np * Np, Np, sA, sD, sW, sT, st));
    if (hipStreamSynchronize(st) != hipSuccess) {
      set_error("model_create: triangular inverse failed: %s", hipGetErrorString(hipGetLastError()));
      return GPEMU_ERR_HIP;
    }
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    set_error("model_create: device synchronisation failed: %s", hipGetErrorString(hipGetLastError()));
    return GPEMU_ERR_HIP;
  }
  return GPEMU_OK;
}

int gpemu_model_create(gpemu_model **out, int device, int64_t N, int64_t d, int64_t F, int64_t k,
                       int kernel_kind, double nu, int has_const, int has_noise,
                       const double *X_train, const double *ls, const double *constv,
                       const double *noise, const double *alpha, const double *L,
                       const double *components, const double *scaler_mean,
                       const double *scaler_scale, const double *cov_unexplained) {
  GP_ARG(out, "out");
  *out = nullptr;
  GP_ARG(N > 0 && d > 0 && F > 0 && k > 0, "N, d, F, k must be positive");
  GP_ARG(d <= DPAD_WIDE, "d > 16 parameters is not supported by this build");
  GP_ARG(k <= 64, "k > 64 principal components is not supported by this build");
  GP_ARG(kernel_kind == GPEMU_KERNEL_RBF || kernel_kind == GPEMU_KERNEL_MATERN, "kernel_kind");
  if (kernel_kind == GPEMU_KERNEL_MATERN) GP_ARG(nu > 0.0, "Matern nu must be > 0 (finite or +inf; not NaN)");
  GP_ARG(X_train && ls && alpha && L && components && scaler_mean && scaler_scale, "null array");
  GP_ARG(!has_const || constv, "constv");
  GP_ARG(!has_noise || noise, "noise");
  GP_TRY(device_ready(device));

  gpemu_model *m = new gpemu_model();
  m->device = device;
  m->N = N; m->d = d; m->F = F; m->k = k;
  m->dp = dpad_of(d);
  m->Npad = round_up(N, TILE);
  m->vsq_nrb = m->Npad / 64;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      m->num_cu = prop.multiProcessorCount;
  }
  m->kernel_kind = kernel_kind; m->nu = nu;
  m->has_const = has_const ? 1 : 0; m->has_noise = has_noise ? 1 : 0;
  const int rc = model_fill(m, X_train, ls, constv, noise, alpha, L, components, scaler_mean, scaler_scale, cov_unexplained);
  if (rc != GPEMU_OK) {
    gpemu_model_destroy(m);
    return rc;
  }
  *out = m;
  return GPEMU_OK;
}

int gpemu_model_destroy(gpemu_model *m) {
  if (!m) return GPEMU_OK;
  hipSetDevice(m->device);
  if (m->stream) hipStreamSynchronize(m->stream);
  dev_free(m->Xs); dev_free(m->inv_ls); dev_free(m->ls); dev_free(m->Xa); dev_free(m->alf); dev_free(m->qsc); dev_free(m->qof);
  dev_free(m->etab); dev_free(m->constv); dev_free(m->kdiag);
  dev_free(m->alpha); dev_free(m->cv_jit); dev_free(m->Wt); dev_free(m->Xtr); dev_free(m->comp); dev_free(m->smean); dev_free(m->sscale);
  dev_free(m->cunexpl); dev_free(m->yexp); dev_free(m->yerr); dev_free(m->lo); dev_free(m->hi);
  for (gpemu_model::LikEntry &en : m->lik_cache) free_lik_entry(en);
  dev_free(m->ycov); dev_free(m->srcs);
  dev_free(m->exact_scratch);
  dev_free(m->grad_ws);
  dev_free(m->grad_lik_ws);
  dev_free(m->blk_start); dev_free(m->blk_of);
  for (gpemu_model::SchedEntry &en : m->sched_cache) { dev_free(en.items); dev_free(en.cnt); }
  for (gpemu_model::SchedEntry &en : m->sm_cache) { dev_free(en.items); dev_free(en.cnt); }
  for (gpemu_model::LiveDeal &en : m->live_cache) { dev_free(en.items); dev_free(en.cnt); dev_free(en.kmap); }
  dev_free(m->lik_terms);
  dev_free(m->lik_tickets);
  dev_free(m->live_cnt);
  free_workspace(m->ws);
  for (hipEvent_t &e : m->ev_pool) event_destroy(e);
  stream_destroy(m->stream);
  delete m;
  return GPEMU_OK;
}

int gpemu_model_profile(gpemu_model *m, int enable) {
  GP_ARG(m, "model");
  GP_HIP(hipSetDevice(m->device));
  GP_HIP(hipDeviceSynchronize());
  prof_drain(m);
  m->profiling = enable != 0;
  m->prof_ms[0] = m->prof_ms[1] = 0.0;
  m->prof_n[0] = m->prof_n[1] = 0;
  GP_HIP(hipMemset(m->live_cnt, 0, sizeof(long long) * 2));
  return GPEMU_OK;
}

int gpemu_model_live_counts(gpemu_model *m, int64_t *live_proposals) {
  GP_ARG(m && live_proposals, "null pointer");
  GP_HIP(hipSetDevice(m->device));
  GP_HIP(hipDeviceSynchronize());
  long long h[2] = {0, 0};
  GP_HIP(hipMemcpy(h, m->live_cnt, sizeof(h), hipMemcpyDeviceToHost));
  live_proposals[0] = h[0];
  live_proposals[1] = h[1];
  return GPEMU_OK;
}

int gpemu_model_profile_read(gpemu_model *m, double *ms_total, int64_t *launches) {
  GP_ARG(m && ms_total && launches, "null pointer");
  GP_HIP(hipSetDevice(m->device));
  GP_HIP(hipDeviceSynchronize());
  prof_drain(m);
  for (int i = 0; i < 2; ++i) { ms_total[i] = m->prof_ms[i]; launches[i] = m->prof_n[i]; }
  return GPEMU_OK;
}

int gpemu_model_dims(const gpemu_model *m, int64_t *N, int64_t *d, int64_t *F, int64_t *k) {
  GP_ARG(m, "model");
  if (N) *N = m->N;
  if (d) *d = m->d;
  if (F) *F = m->F;
  if (k) *k = m->k;
  return GPEMU_OK;
}

int gpemu_model_device(const gpemu_model *m) { return m ? m->device : GPEMU_ERR_ARG; }

int gpemu_model_sync(gpemu_model *m) {
  GP_ARG(m, "model");
  GP_HIP(hipSetDevice(m->device));
  GP_HIP(hipStreamSynchronize(m->stream));
  return GPEMU_OK;
}

// ---- GP predict --------------------------------------------------------------------------------
constexpr int64_t MAX_CHUNK = 2048;   // rows per pass of the predict pipeline (bounds the K_* workspace)

// caller rows [B][d]: the cross-kernel kernel pads them into the workspace itself
static ProposeArgs raw_rows(const gpemu_model *m, int64_t B, const double *dX) {
  ProposeArgs raw;
  raw.raw = dX; raw.n = (int)B; raw.d = (int)m->d;
  return raw;
}

static int gp_predict_core(gpemu_model *m, int64_t B, const double *dX, hipStream_t st) {
  GP_TRY(ensure_workspace(m, B));
  const ProposeArgs raw = raw_rows(m, B, dX);
  GP_TRY(launch_kstar(m, B, m->ws.Xq, st, &raw));
  GP_TRY(launch_trmm_vsq(m, B, st));
  return GPEMU_OK;
}


int gpemu_gp_predict_dev(gpemu_model *m, int64_t B, const double *dX, double *dmean, double *dvar,
                         void *stream) {
  GP_ARG(m && dX && dmean && dvar, "null pointer");
  GP_ARG(B > 0, "B must be positive");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  for (int64_t off = 0; off < B; off += MAX_CHUNK) {   // large batches go through in chunks
    const int64_t nb = (B - off < MAX_CHUNK) ? (B - off) : MAX_CHUNK;
    path_count(GPEMU_PATH_PREDICT_PASS);
    GP_TRY(gp_predict_core(m, nb, dX + off * m->d, st));
    GP_TRY(launch_reduce_mean_var(m, nb, dmean + off * m->k, dvar + off * m->k, st));
  }
  return GPEMU_OK;
}

int gpemu_gp_predict(gpemu_model *m, int64_t B, const double *X, double *mean_out, double *var_out) {
  GP_ARG(m && X && mean_out && var_out, "null pointer");
  GP_ARG(B > 0, "B must be positive");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  DevScope sc(st);
  double *dX = nullptr, *dm = nullptr, *dv = nullptr;
  GP_TRY(sc.alloc(&dX, B * m->d));
  GP_TRY(sc.alloc(&dm, B * m->k));
  GP_TRY(sc.alloc(&dv, B * m->k));
  GP_TRY(upload(dX, X, B * m->d, st));
  GP_TRY(gpemu_gp_predict_dev(m, B, dX, dm, dv, st));
  GP_TRY(sc.download(mean_out, dm, B * m->k));
  GP_TRY(sc.download(var_out, dv, B * m->k));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

// ---- joint predictive covariance and draws (k_pcov.hip) --------------------------------------------------
static bool all_finite(const double *x, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) return false;
  return true;
}

int gpemu_gp_predict_cov_dev(gpemu_model *m, int64_t M1, const double *dX1, int64_t M2, const double *dX2,
                             int64_t workspace_bytes, double *dmean, double *dcov, void *stream) {
  GP_ARG(m && dX1 && dcov, "null pointer");
  GP_ARG(M1 > 0, "M1 must be positive");
  GP_ARG(!dX2 || M2 > 0, "M2 must be positive");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  if (dmean) {
    // the mean through gp_predict's own launches: the same bits
    DevScope sc(st);
    double *dvar = nullptr;
    GP_TRY(sc.alloc(&dvar, M1 * m->k));
    GP_TRY(gpemu_gp_predict_dev(m, M1, dX1, dmean, dvar, st));
    if (hipStreamSynchronize(st) != hipSuccess) {
      set_error("gp_predict_cov: %s", hipGetErrorString(hipGetLastError()));
      return GPEMU_ERR_HIP;
    }
  }
  return predict_cov(m, M1, dX1, dX2 ? M2 : M1, dX2, workspace_bytes, dcov, st);
}

int gpemu_gp_predict_cov(gpemu_model *m, int64_t M1, const double *X1, int64_t M2, const double *X2,
                         int64_t workspace_bytes, double *mean_out, double *cov_out) {
  GP_ARG(m && X1 && cov_out, "null pointer");
  GP_ARG(M1 > 0, "M1 must be positive");
  GP_ARG(!X2 || M2 > 0, "M2 must be positive");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_ARG(all_finite(X1, M1 * m->d) && (!X2 || all_finite(X2, M2 * m->d)), "X contains NaN or infinity");
  if (!X2) M2 = M1;
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  DevScope sc(st);
  double *dX1 = nullptr, *dX2 = nullptr, *dm = nullptr, *dc = nullptr;
  GP_TRY(sc.alloc(&dX1, M1 * m->d));
  if (X2) GP_TRY(sc.alloc(&dX2, M2 * m->d));
  if (mean_out) GP_TRY(sc.alloc(&dm, M1 * m->k));
  GP_TRY(sc.alloc(&dc, m->k * M1 * M2));
  GP_TRY(upload(dX1, X1, M1 * m->d, st));
  if (X2) GP_TRY(upload(dX2, X2, M2 * m->d, st));
  GP_TRY(gpemu_gp_predict_cov_dev(m, M1, dX1, M2, dX2, workspace_bytes, dm, dc, st));
  GP_TRY(sc.download(cov_out, dc, m->k * M1 * M2));
  if (mean_out) GP_TRY(sc.download(mean_out, dm, M1 * m->k));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_gp_sample(gpemu_model *m, int64_t M, const double *X, int64_t n_draws, const double *z,
                    double *draws_out, double *tau_out) {
  GP_ARG(m && X && z && draws_out && tau_out, "null pointer");
  GP_ARG(M > 0, "M must be positive");
  GP_ARG(n_draws > 0, "n_draws must be positive");
  GP_ARG(all_finite(X, M * m->d), "X contains NaN or infinity");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int64_t k = m->k;
  DevScope sc(st);
  double *dX = nullptr, *dm = nullptr, *dc = nullptr, *dz = nullptr, *dout = nullptr;
  GP_TRY(sc.alloc(&dX, M * m->d));
  GP_TRY(sc.alloc(&dm, M * k));
  GP_TRY(sc.alloc(&dc, k * M * M));
  GP_TRY(sc.alloc(&dz, k * M * n_draws));
  GP_TRY(sc.alloc(&dout, k * M * n_draws));
  GP_TRY(upload(dX, X, M * m->d, st));
  GP_TRY(upload(dz, z, k * M * n_draws, st));
  GP_TRY(gpemu_gp_predict_cov_dev(m, M, dX, 0, nullptr, 0, dm, dc, st));
  const int rc = sample_from_cov(m, M, n_draws, dc, dm, dz, dout, tau_out, st);
  if (rc < GPEMU_OK) return rc;
  // a PC whose ladder ran out (rc > 0): the others' draws are still returned
  GP_TRY(sc.download(draws_out, dout, k * M * n_draws));
  GP_HIP(hipStreamSynchronize(st));
  return rc;
}

// ---- cross-validation (k_cv.hip) -----------------------------------------------------------------------
int gpemu_model_cross_validate(gpemu_model *m, int64_t n_folds, const int32_t *fold, const double *y_train,
                               double *mean_pc, double *var_pc, double *central_value, double *variance) {
  GP_ARG(m && fold && y_train && mean_pc && var_pc, "null pointer");
  const int64_t N = m->N, k = m->k;
  GP_ARG(n_folds >= 2 && n_folds <= N, "n_folds must be in [2, N]");
  std::vector<int> cnt((size_t)n_folds + 1, 0);
  for (int64_t i = 0; i < N; ++i) {
    GP_ARG(fold[i] >= 0 && fold[i] < n_folds, "fold label out of [0, n_folds)");
    ++cnt[(size_t)fold[i] + 1];
  }
  for (int64_t f = 0; f < n_folds; ++f) GP_ARG(cnt[(size_t)f + 1] > 0, "empty fold");
  // the points of every fold, ascending, fold after fold; hfoff = fold offsets, hr0 = first point of each fold
  std::vector<int> hfoff((size_t)n_folds + 1, 0), hr0((size_t)n_folds), hidx((size_t)N);
  for (int64_t f = 0; f < n_folds; ++f) hfoff[(size_t)f + 1] = hfoff[(size_t)f] + cnt[(size_t)f + 1];
  {
    std::vector<int> pos(hfoff.begin(), hfoff.end() - 1);
    for (int64_t i = 0; i < N; ++i) hidx[(size_t)pos[(size_t)fold[i]]++] = (int)i;
  }
  for (int64_t f = 0; f < n_folds; ++f) hr0[(size_t)f] = hidx[(size_t)hfoff[(size_t)f]];
  // tests: the largest number of (PC, fold) problems per chunk; read once per call
  const char *cap_env = getenv("GPEMU_CV_CHUNK");
  const int64_t max_chunk = cap_env ? atoll(cap_env) : 0;
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  DevScope sc(st);
  int *didx = nullptr, *dfoff = nullptr;
  double *dy = nullptr, *dm = nullptr, *dv = nullptr, *dcv = nullptr, *dvo = nullptr;
  GP_TRY(sc.alloc(&didx, N));
  GP_TRY(sc.alloc(&dfoff, n_folds + 1));
  GP_TRY(sc.alloc(&dy, N * k));
  GP_TRY(sc.alloc(&dm, N * k));
  GP_TRY(sc.alloc(&dv, N * k));
  if (central_value) GP_TRY(sc.alloc(&dcv, N * m->F));
  if (variance) GP_TRY(sc.alloc(&dvo, N * m->F));
  GP_TRY(upload(didx, hidx.data(), N, st));
  GP_TRY(upload(dfoff, hfoff.data(), n_folds + 1, st));
  GP_TRY(upload(dy, y_train, N * k, st));
  GP_TRY(cross_validate(m, (int)n_folds, didx, dfoff, hfoff, hr0, dy, dm, dv, max_chunk));
  GP_TRY(launch_cv_backproject(m, dm, dv, dcv, dvo));
  GP_TRY(sc.download(mean_pc, dm, N * k));
  GP_TRY(sc.download(var_pc, dv, N * k));
  if (dcv) GP_TRY(sc.download(central_value, dcv, N * m->F));
  if (dvo) GP_TRY(sc.download(variance, dvo, N * m->F));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

// ---- likelihood ----------------------------------------------------------------------------------
int gpemu_likelihood_setup(gpemu_model *m, const double *y_exp, const double *y_err,
                           const double *lo, const double *hi, double n_div, int64_t n_blocks,
                           const int64_t *block_start) {
  return gpemu_likelihood_setup_chains(m, 1, y_exp, y_err, lo, hi, n_div, n_blocks, block_start);
}

int gpemu_likelihood_setup_chains(gpemu_model *m, int n_chains, const double *y_exp, const double *y_err,
                                  const double *lo, const double *hi, double n_div, int64_t n_blocks,
                                  const int64_t *block_start) {
  return gpemu_likelihood_setup_cov(m, n_chains, y_exp, y_err, nullptr, 0, nullptr, lo, hi, n_div, n_blocks, block_start);
}

int gpemu_likelihood_setup_cov(gpemu_model *m, int n_chains, const double *y_exp, const double *y_err,
                               const double *cov, int64_t n_src, const double *sources, const double *lo,
                               const double *hi, double n_div, int64_t n_blocks, const int64_t *block_start) {
  GP_ARG(m && y_exp && y_err && lo && hi, "null pointer");
  GP_ARG(n_div >= 1.0, "n_div must be >= 1");
  GP_ARG(n_chains >= 1 && n_chains <= 4096, "n_chains must be in [1, 4096]");
  GP_ARG(n_src >= 0 && n_src <= GPEMU_MAX_SOURCES, "n_src must be in [0, 16]");
  GP_ARG(n_src == 0 || sources, "sources");
  const int64_t NC = n_chains, S = n_src;
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int64_t F = m->F, k = m->k;
  // observable blocks (default: one block = the whole group)
  std::vector<int> hstart, hof((size_t)F, 0);
  if (n_blocks <= 0 || !block_start) {
    hstart = {0, (int)F};
  } else {
    GP_ARG(block_start[0] == 0 && block_start[n_blocks] == F, "block_start must cover [0, F]");
    for (int64_t o = 0; o <= n_blocks; ++o) {
      if (o > 0) GP_ARG(block_start[o] > block_start[o - 1], "block_start must be increasing");
      hstart.push_back((int)block_start[o]);
    }
  }
  const int64_t nblk = (int64_t)hstart.size() - 1;
  for (int64_t o = 0; o < nblk; ++o)
    for (int f = hstart[o]; f < hstart[o + 1]; ++f) hof[f] = (int)o;
  if (cov) {
    // C_d's dense part lives inside the observables: the likelihood factorises over the blocks (the sources carry what
    // is correlated across them)
    for (int64_t f = 0; f < F; ++f)
      for (int64_t g = 0; g < F; ++g) {
        const double v = cov[f * F + g];
        if (v != cov[g * F + f] || !std::isfinite(v)) {
          set_error("bad argument: cov must be finite and symmetric (entry %lld, %lld)", (long long)f, (long long)g);
          return GPEMU_ERR_ARG;
        }
        if (hof[f] != hof[g] && v != 0.0) {
          set_error("bad argument: cov[%lld][%lld] = %g couples observable blocks %d and %d: give correlations across "
                    "observables as sources", (long long)f, (long long)g, v, hof[f], hof[g]);
          return GPEMU_ERR_ARG;
        }
      }
  }
  GP_ARG(S == 0 || all_finite(sources, S * F), "sources must be finite");
  // same data as the cached constants belong to?  then an n_div seen before is a pointer swap
  std::vector<double> key;
  key.push_back((double)NC);
  key.insert(key.end(), y_exp, y_exp + NC * F);
  key.insert(key.end(), y_err, y_err + F);
  key.insert(key.end(), lo, lo + m->d);
  key.insert(key.end(), hi, hi + m->d);
  for (int v : hstart) key.push_back((double)v);
  key.push_back(cov ? 1.0 : 0.0);
  if (cov) key.insert(key.end(), cov, cov + F * F);
  key.push_back((double)S);
  key.insert(key.end(), sources, sources + S * F);
  const bool same_data = m->lik_ready && key.size() == m->lik_host.size() &&
                         memcmp(key.data(), m->lik_host.data(), sizeof(double) * key.size()) == 0;
  if (same_data) {
    for (const gpemu_model::LikEntry &en : m->lik_cache)
      if (en.n_div == n_div) {
        GP_HIP(hipStreamSynchronize(st));
        m->G = en.G; m->g0 = en.g0; m->scal = en.scal; m->W = en.W; m->Q = en.Q; m->w0 = en.w0; m->n_div = n_div;
        return GPEMU_OK;
      }
  } else {
    GP_HIP(hipStreamSynchronize(st));
    for (gpemu_model::LikEntry &en : m->lik_cache) free_lik_entry(en);
    m->lik_cache.clear();
    m->G = m->g0 = m->scal = m->W = m->Q = m->w0 = nullptr;
  }
  // from here on the fields of the setup change one by one: until the last of them is in place the handle has no
  // likelihood, so that a failure half way (an allocation, a matrix that is not positive definite) leaves a handle that
  // says so and takes the next setup from scratch, not one whose launches read a freed or null field
  m->lik_ready = false;
  m->lik_host.clear();
  if (m->lik_cache.size() >= 64) {           // bounded: drop the oldest entry
    GP_HIP(hipStreamSynchronize(st));
    free_lik_entry(m->lik_cache.front());
    m->lik_cache.erase(m->lik_cache.begin());
  }
  GP_HIP(hipStreamSynchronize(st));
  // (each on its own: an earlier setup may have ended between two of them)
  if (!m->yerr) GP_TRY(dev_alloc(&m->yerr, F));
  if (!m->lo) GP_TRY(dev_alloc(&m->lo, m->dp));
  if (!m->hi) GP_TRY(dev_alloc(&m->hi, m->dp));
  if (!m->blk_of) GP_TRY(dev_alloc(&m->blk_of, F));
  dev_free(m->yexp);
  GP_TRY(dev_alloc(&m->yexp, NC * F));
  m->lik_chains = n_chains;
  dev_free(m->blk_start);
  dev_free(m->ycov);
  dev_free(m->srcs);
  m->n_src = 0;
  if (cov) GP_TRY(dev_alloc(&m->ycov, F * F));
  if (S > 0) GP_TRY(dev_alloc(&m->srcs, S * F));
  m->n_src = (int)S;
  // the new cache entry belongs to a scope until it is complete: a failure half way leaves nothing behind
  gpemu_model::LikEntry en{n_div, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  {
    DevScope entry(st);
    GP_TRY(entry.alloc(&en.G, nblk * k * k)); GP_TRY(entry.alloc(&en.g0, NC * nblk * k));
    GP_TRY(entry.alloc(&en.scal, NC * 2 * nblk)); GP_TRY(dev_alloc(&m->blk_start, nblk + 1));
    if (S > 0) {
      GP_TRY(entry.alloc(&en.W, nblk * k * S)); GP_TRY(entry.alloc(&en.Q, nblk * S * S)); GP_TRY(entry.alloc(&en.w0, NC * nblk * S));
    }
    for (double *p : {en.G, en.g0, en.scal, en.W, en.Q, en.w0}) entry.release(p);
  }
  m->G = en.G; m->g0 = en.g0; m->scal = en.scal; m->W = en.W; m->Q = en.Q; m->w0 = en.w0;
  m->lik_cache.push_back(en);
  m->nblk = nblk;
  GP_HIP(hipMemcpyAsync(m->blk_start, hstart.data(), sizeof(int) * (nblk + 1), hipMemcpyHostToDevice, st));
  GP_HIP(hipMemcpyAsync(m->blk_of, hof.data(), sizeof(int) * F, hipMemcpyHostToDevice, st));
  m->n_div = n_div;
  double hlo[DPAD_WIDE], hhi[DPAD_WIDE];
  for (int i = 0; i < m->dp; ++i) { hlo[i] = i < m->d ? lo[i] : -INFINITY; hhi[i] = i < m->d ? hi[i] : INFINITY; }
  GP_TRY(upload(m->yexp, y_exp, NC * F, st)); GP_TRY(upload(m->yerr, y_err, F, st));
  GP_TRY(upload(m->lo, hlo, m->dp, st)); GP_TRY(upload(m->hi, hhi, m->dp, st));
  if (cov) GP_TRY(upload(m->ycov, cov, F * F, st));
  if (S > 0) GP_TRY(upload(m->srcs, sources, S * F, st));
  GP_HIP(hipStreamSynchronize(st));  // hlo/hhi are stack buffers
  std::vector<int> info((size_t)nblk, 0);
  {
    DevScope sc(st);
    double *dA = nullptr, *dPT = nullptr, *dZ = nullptr;
    int *dinfo = nullptr;
    GP_TRY(sc.alloc(&dA, F * F));
    GP_TRY(sc.alloc(&dPT, nblk * chol_scratch_size(F)));
    GP_TRY(sc.alloc(&dZ, F * (k + NC + S)));
    GP_TRY(sc.alloc(&dinfo, nblk));
    GP_HIP(hipMemsetAsync(dinfo, 0, sizeof(int) * nblk, st));
    GP_TRY(launch_lik_setup(m, hstart, dA, dPT, dZ, dinfo, st));
    GP_TRY(sc.download(info.data(), dinfo, nblk));
    GP_HIP(hipStreamSynchronize(st));
  }
  for (int64_t o = 0; o < nblk; ++o) {
    if (info[o] != 0) {
      set_error("likelihood_setup: A = C_unexpl/n o ss^T + %s is not positive definite "
                "(observable block %lld, pivot %d)", cov ? "cov" : "diag(y_err^2)", (long long)o, info[o]);
      return hstart[o] + info[o];
    }
  }
  m->lik_ready = true;
  m->lik_host = key;
  if (cov) src_path_count(GPEMU_SRC_PATH_SETUP_COV);
  if (S > 0) src_path_count(GPEMU_SRC_PATH_SETUP_SOURCES);
  return GPEMU_OK;
}

int gpemu_logpost_dev(gpemu_model *m, int64_t B, const double *dX, double *dout, int mode, void *stream) {
  GP_ARG(m, "null pointer");
  GP_ARG(B >= 0, "B must not be negative");
  if (B == 0) return GPEMU_OK;   /* empty batch -> empty result (ref: log_posterior.py:59,68) */
  GP_ARG(dX && dout, "null pointer");
  GP_TRY(logpost_mode_ready(m, mode));
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  const LaunchSwitches sw = read_launch_switches();
  for (int64_t off = 0; off < B; off += MAX_CHUNK) {
    const int64_t nb = (B - off < MAX_CHUNK) ? (B - off) : MAX_CHUNK;
    path_count(GPEMU_PATH_PREDICT_PASS);
    if (mode == GPEMU_LOGPOST_LOWRANK) {
      GP_TRY(ensure_workspace(m, nb));   // (before ws.Xq is read: it may move)
      const ProposeArgs raw = raw_rows(m, nb, dX + off * m->d);
      GP_TRY(logpost_eval(&m, 1, nb, m->ws.Xq, dout + off, st, sw, nullptr, &raw));
    } else {
      GP_TRY(gp_predict_core(m, nb, dX + off * m->d, st));
      GP_TRY(launch_loglik_exact(m, nb, m->ws.Xq, dout + off, st));
    }
  }
  return GPEMU_OK;
}

int gpemu_logpost(gpemu_model *m, int64_t B, const double *X, double *out, int mode) {
  GP_ARG(m, "null pointer");
  GP_ARG(B >= 0, "B must not be negative");
  if (B == 0) return GPEMU_OK;
  GP_ARG(X && out, "null pointer");
  GP_TRY(logpost_mode_ready(m, mode));
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  DevScope sc(st);
  double *dX = nullptr, *dout = nullptr;
  GP_TRY(sc.alloc(&dX, B * m->d));
  GP_TRY(sc.alloc(&dout, B));
  GP_TRY(upload(dX, X, B * m->d, st));
  GP_TRY(gpemu_logpost_dev(m, B, dX, dout, mode, st));
  GP_TRY(sc.download(out, dout, B));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_logpost_groups(gpemu_model *const *models, int n_groups, int64_t B, const double *X, double *out, int mode) {
  GP_ARG(models && n_groups > 0, "models");
  GP_ARG(B >= 0, "B must not be negative");
  GP_ARG(mode == GPEMU_LOGPOST_LOWRANK || mode == GPEMU_LOGPOST_EXACT, "mode");
  for (int g = 0; g < n_groups; ++g) {
    GP_ARG(models[g], "null model");
    GP_ARG(models[g]->d == models[0]->d && models[g]->device == models[0]->device,
           "models must share the parameter dimension and the device");
  }
  if (B == 0) return GPEMU_OK;
  GP_ARG(X && out, "null pointer");
  gpemu_model *m0 = models[0];
  if (mode == GPEMU_LOGPOST_EXACT) {
    // validation form: the groups one after the other, their terms added in group order on the host
    std::vector<double> part((size_t)B);
    for (int g = 0; g < n_groups; ++g) {
      GP_TRY(gpemu_logpost(models[g], B, X, g == 0 ? out : part.data(), mode));
      if (g > 0)
        for (int64_t i = 0; i < B; ++i) out[i] = part[(size_t)i] + out[i];
    }
    return GPEMU_OK;
  }
  GP_TRY(logpost_groups_ready(models, n_groups));
  GP_HIP(hipSetDevice(m0->device));
  hipStream_t st = m0->stream;
  const LaunchSwitches sw = read_launch_switches();
  DevScope sc(st);
  double *dX = nullptr, *dout = nullptr;
  GP_TRY(sc.alloc(&dX, B * m0->d));
  GP_TRY(sc.alloc(&dout, B));
  GP_TRY(upload(dX, X, B * m0->d, st));
  for (int64_t off = 0; off < B; off += MAX_CHUNK) {
    const int64_t nb = (B - off < MAX_CHUNK) ? (B - off) : MAX_CHUNK;
    path_count(GPEMU_PATH_PREDICT_PASS);
    GP_TRY(ensure_workspace(m0, nb));   // (before ws.Xq is read: it may move)
    const ProposeArgs raw = raw_rows(m0, nb, dX + off * m0->d);
    GP_TRY(logpost_eval(models, n_groups, nb, m0->ws.Xq, dout + off, st, sw, nullptr, &raw));
  }
  GP_TRY(sc.download(out, dout, B));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

// ---- truncation covariance -----------------------------------------------------------------------
}  // extern "C"
namespace gpemu {
// rows n_pc.. of the components, zero padded to [Kp][Fp]: A plain, Bm scaled by the row's explained variance
__global__ void trunc_pack_kernel(const double *__restrict__ comp, const double *__restrict__ ev, double *__restrict__ A,
                                  double *__restrict__ Bm, int F, int Fp, int K, int Kp, int n_pc) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)Kp * Fp) return;
  const int r = (int)(idx / Fp), f = (int)(idx - (int64_t)r * Fp);
  double v = 0.0, lam = 0.0;
  if (r < K && f < F) { v = comp[(int64_t)(n_pc + r) * F + f]; lam = ev[n_pc + r]; }
  A[idx] = v;
  Bm[idx] = lam * v;
}
}  // namespace gpemu
extern "C" {

int gpemu_truncation_cov(int device, int64_t n_comp, int64_t F, int64_t n_pc, const double *components,
                         const double *explained_variance, double *cov_out) {
  GP_ARG(components && explained_variance && cov_out, "null pointer");
  GP_ARG(n_comp > 0 && F > 0 && n_pc >= 0 && n_pc <= n_comp, "n_comp, F, n_pc");
  GP_TRY(device_ready(device));
  const int64_t K = n_comp - n_pc;
  if (K == 0) {
    memset(cov_out, 0, sizeof(double) * (size_t)(F * F));
    return GPEMU_OK;
  }
  const int64_t Fp = round_up(F, 64), Kp = round_up(K, 32);
  double *dcomp = nullptr, *dev_ = nullptr, *dA = nullptr, *dB = nullptr, *dC = nullptr;
  hipStream_t st = nullptr;   // a one-off setup product: the null stream
  DevScope sc(st);
  GP_TRY(sc.alloc(&dcomp, n_comp * F));
  GP_TRY(sc.alloc(&dev_, n_comp));
  GP_TRY(sc.alloc(&dA, Kp * Fp));
  GP_TRY(sc.alloc(&dB, Kp * Fp));
  GP_TRY(sc.alloc(&dC, Fp * Fp));
  GP_TRY(upload(dcomp, components, n_comp * F, st));
  GP_TRY(upload(dev_, explained_variance, n_comp, st));
  const int64_t n = Kp * Fp;
  hipLaunchKernelGGL(trunc_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dcomp, dev_, dA, dB,
                     (int)F, (int)Fp, (int)K, (int)Kp, (int)n_pc);
  GemmArgs g;                       // C[f][g] = sum_r A[r][f] * (lambda_r A[r][g]): both operands k-major
  g.A = dA; g.B = dB; g.C = dC;
  g.lda = Fp; g.ldb = Fp; g.ldc = Fp;
  g.M = (int)Fp; g.N = (int)Fp; g.K = (int)Kp;
  GP_TRY(launch_gemm(g, true, true, 1, st));
  GP_HIP(hipMemcpy2DAsync(cov_out, sizeof(double) * F, dC, sizeof(double) * Fp, sizeof(double) * F, (size_t)F,
                          hipMemcpyDeviceToHost, st));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

// ---- full predict ----------------------------------------------------------------------------------
int gpemu_predict_full_dev(gpemu_model *m, int64_t B, const double *dX, double n_div, double *dcv,
                           double *dcov, void *stream) {
  GP_ARG(m && dX && dcv && dcov, "null pointer");
  GP_ARG(B > 0 && n_div >= 1.0, "B, n_div");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  const int64_t F = m->F;
  for (int64_t off = 0; off < B; off += MAX_CHUNK) {
    const int64_t nb = (B - off < MAX_CHUNK) ? (B - off) : MAX_CHUNK;
    path_count(GPEMU_PATH_PREDICT_PASS);
    GP_TRY(gp_predict_core(m, nb, dX + off * m->d, st));
    // no mean / variance arrays: the writer sums the GP stage's partials itself (one launch less)
    GP_TRY(launch_predict_full(m, nb, n_div, dcv + off * F, dcov + off * F * F, st, nullptr, nullptr));
  }
  return GPEMU_OK;
}

int gpemu_predict_full(gpemu_model *m, int64_t B, const double *X, double n_div, double *cv_out,
                       double *cov_out) {
  GP_ARG(m && X && cv_out && cov_out, "null pointer");
  GP_ARG(B > 0, "B must be positive");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int64_t F = m->F;
  DevScope sc(st);
  double *dX = nullptr, *dcv = nullptr, *dcov = nullptr;
  GP_TRY(sc.alloc(&dX, B * m->d));
  GP_TRY(sc.alloc(&dcv, B * F));
  GP_TRY(sc.alloc(&dcov, B * F * F));
  GP_TRY(upload(dX, X, B * m->d, st));
  GP_TRY(gpemu_predict_full_dev(m, B, dX, n_div, dcv, dcov, st));
  GP_TRY(sc.download(cv_out, dcv, B * F));
  GP_TRY(sc.download(cov_out, dcov, B * F * F));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

}  // extern "C"
