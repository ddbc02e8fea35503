// Hamiltonian Monte Carlo on the device: W independent chains advance in lock step, one chain per
// "walker" of the sampler's chain layout, on the analytic gradient of the log-posterior (k_grad.hip).
//
// One iteration of chain w (tests/hmc_ref.py restates it in numpy and is the specification):
//     eps_w = eps (1 + jitter (2 u_j - 1)),   p = z / sqrt(minv),   K_old = 1/2 sum minv p^2
//     L times:  p += 1/2 eps_w g;  x += eps_w minv p;  reflect (x, p) at the prior's faces;  g = grad lp(x);  p += 1/2 eps_w g
//     H = -lp + K;  accept iff log u < H_old - H_new;  a non-finite H_new, or H_new - H_old > 1000, away from a face is a
//     rejected divergence;  on reject x, lp and g stay
// The gradient of the current state is carried from iteration to iteration: L gradient evaluations per iteration.
// Randomness: Philox4x32-10, counter (w, tag, step_lo, step_hi), key = the sampler's seed (tags 0 .. 5: k_sampler.hip,
// k_temper.hip).  Tag 6: words x, y -> the accept uniform, words z, w -> the step jitter.  Tag 8 + j: the normal pair
// (2j, 2j + 1) by Box-Muller, u1 = u01(x, y), u2 = u01(z, w):
//     rad = sqrt(-2 log(1 - u1)),  z_2j = rad cos(2 pi u2),  z_2j+1 = rad sin(2 pi u2)
// Launches per iteration: begin (draw, first kick, drift, reflect), then L gradient evaluations with a fused
// kick-kick-drift-reflect between them, finish (last kick, energies, accept, counters, state and chain row), adapt (the
// mean accept probability over the chains in a fixed order and the dual-averaging update of the step size).  Everything
// is ordered by the sampler's stream: the step size is read and written on the device, the host reads nothing in a run.
// No float atomics.
#include "internal.h"
#include "rows_dev.h"
#include "sampler_internal.h"
#include "wg_dev.h"

#include <algorithm>
#include <cmath>

namespace gpemu {

static inline void hmc_path_count(int path) { count_path(PATHS_HMC, path); }

// the adaptation state on the device (HmcState::ad)
enum { AD_EPS = 0, AD_LOG_EPS_BAR, AD_HBAR, AD_M, AD_MU, AD_LAST, AD_SUM, AD_N, AD_COUNT };
// dual averaging (Hoffman & Gelman 2014, algorithm 5): gpemu/hmc.py and tests/hmc_ref.py hold the same constants
constexpr double DA_GAMMA = 0.05, DA_T0 = 10.0, DA_KAPPA = 0.75;
constexpr double HMC_DIVERGENT = 1000.0;
constexpr int HMC_MAX_D = DPAD_WIDE;

struct HmcArgs {
  double *X, *logp, *g;              // the chains' states: [W][dp], [W], [W][d]
  double *xq, *p, *gnew, *lpnew;     // the trajectory: [W][d], [W][d], [W][d], [W]
  double *kin0, *epsw, *logu, *accp; // [W]
  const double *minv, *lo, *hi, *ad;
  long long *naccept, *ndiv;
  int *flags;
  double *chain, *lpchain;           // this iteration's row, or null
  int W, d, dp;
};

// closed-form reflection at the faces lo, hi (Neal 2011, 5.1): any number of bounces costs the same
__device__ __forceinline__ void hmc_reflect(double &x, double &p, double lo, double hi) {
  const double w = hi - lo, w2 = 2.0 * w;
  double t = fmod(x - lo, w2);
  if (t < 0.0) t += w2;
  const bool back = t > w;
  x = lo + (back ? w2 - t : t);
  if (back) p = -p;
}

__device__ __forceinline__ void hmc_normal_pair(uint32_t w, int j, uint32_t step_lo, uint32_t step_hi, uint32_t k0,
                                                uint32_t k1, double &z0, double &z1) {
  const u32x4 r = philox4x32_10(u32x4{w, (uint32_t)(8 + j), step_lo, step_hi}, k0, k1);
  const double u1 = u01_from(r.x, r.y), u2 = u01_from(r.z, r.w);
  const double rad = sqrt(-2.0 * log(1.0 - u1));
  double sn, cs;
  sincos(6.283185307179586 * u2, &sn, &cs);
  z0 = rad * cs;
  z1 = rad * sn;
}

// One thread per chain.  HOST: p, log u and eps_w were uploaded (gpemu_sampler_hmc_step_host_rng); else drawn here.
template <bool HOST>
__global__ __launch_bounds__(256) void hmc_begin_kernel(HmcArgs a, uint32_t k0, uint32_t k1, uint32_t step_lo,
                                                        uint32_t step_hi, double jitter) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.W) return;
  double eps;
  if (HOST) {
    eps = a.epsw[w];
  } else {
    const u32x4 r = philox4x32_10(u32x4{(uint32_t)w, 6u, step_lo, step_hi}, k0, k1);
    a.logu[w] = log(u01_from(r.x, r.y));
    eps = a.ad[AD_EPS] * (1.0 + jitter * (2.0 * u01_from(r.z, r.w) - 1.0));
    a.epsw[w] = eps;
  }
  double kin = 0.0;
  for (int j = 0; 2 * j < a.d; ++j) {
    double z[2] = {0.0, 0.0};
    if (!HOST) hmc_normal_pair((uint32_t)w, j, step_lo, step_hi, k0, k1, z[0], z[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int dd = 2 * j + h;
      if (dd >= a.d) break;
      const double mi = a.minv[dd];
      const int64_t at = (int64_t)w * a.d + dd;
      double pp = HOST ? a.p[at] : z[h] / sqrt(mi);
      kin += mi * pp * pp;
      pp += 0.5 * eps * a.g[at];
      double x = a.X[(int64_t)w * a.dp + dd] + eps * mi * pp;
      hmc_reflect(x, pp, a.lo[dd], a.hi[dd]);
      a.xq[at] = x;
      a.p[at] = pp;
    }
  }
  a.kin0[w] = 0.5 * kin;
}

// between two gradient evaluations: the kick that ends a leapfrog step, the one that starts the next, drift, reflection
__global__ __launch_bounds__(256) void hmc_leapfrog_kernel(HmcArgs a) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.W) return;
  const double eps = a.epsw[w];
  for (int dd = 0; dd < a.d; ++dd) {
    const int64_t at = (int64_t)w * a.d + dd;
    const double gg = a.gnew[at], mi = a.minv[dd];
    double pp = a.p[at];
    pp += 0.5 * eps * gg;
    pp += 0.5 * eps * gg;
    double x = a.xq[at] + eps * mi * pp;
    hmc_reflect(x, pp, a.lo[dd], a.hi[dd]);
    a.xq[at] = x;
    a.p[at] = pp;
  }
}

// the last kick, the energies, accept / reject, the counters, the new state and the chain row
__global__ __launch_bounds__(256) void hmc_finish_kernel(HmcArgs a) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.W) return;
  const double eps = a.epsw[w];
  double kin = 0.0;
  for (int dd = 0; dd < a.d; ++dd) {
    const int64_t at = (int64_t)w * a.d + dd;
    const double pp = a.p[at] + 0.5 * eps * a.gnew[at];
    kin += a.minv[dd] * pp * pp;
  }
  kin *= 0.5;
  const double lp0 = a.logp[w], lp1 = a.lpnew[w];
  if (lp1 != lp1) atomicAdd(a.flags, 1);
  const double h0 = -lp0 + a.kin0[w], h1 = -lp1 + kin;
  const double dh = h0 - h1;
  // a point on a face (lp = -inf) is the ordinary reject; anything else that is not finite, or an energy error beyond
  // HMC_DIVERGENT, is a divergence
  const bool div = lp1 != -INFINITY && (!__builtin_isfinite(h1) || h1 - h0 > HMC_DIVERGENT);
  const bool acc = !div && (a.logu[w] < dh);
  a.accp[w] = (div || dh != dh) ? 0.0 : (dh >= 0.0 ? 1.0 : exp(dh));
  if (div) a.ndiv[w] += 1;
  for (int dd = 0; dd < a.d; ++dd) {
    const int64_t at = (int64_t)w * a.d + dd;
    double v = a.X[(int64_t)w * a.dp + dd];
    if (acc) {
      v = a.xq[at];
      a.X[(int64_t)w * a.dp + dd] = v;
      a.g[at] = a.gnew[at];
    }
    if (a.chain) a.chain[at] = v;
  }
  if (acc) {
    a.logp[w] = lp1;
    a.naccept[w] += 1;
  }
  if (a.lpchain) a.lpchain[w] = acc ? lp1 : lp0;
}

// one workgroup: the iteration's mean accept probability (thread t adds the elements t, t + 256, ..., then tree A of
// wg_dev.h), and (adapt) the dual-averaging update
__global__ __launch_bounds__(256) void hmc_adapt_kernel(const double *accp, int W, double *ad, int adapt, double target) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < W; i += 256) s += accp[i];
  s = wg_sum_a<256>(s, red);
  if (threadIdx.x != 0) return;
  const double mean = s / (double)W;
  ad[AD_LAST] = mean;
  ad[AD_SUM] += mean;
  ad[AD_N] += 1.0;
  if (adapt) {
    const double m = ad[AD_M] + 1.0, wt = 1.0 / (m + DA_T0);
    const double hbar = (1.0 - wt) * ad[AD_HBAR] + wt * (target - mean);
    const double le = ad[AD_MU] - sqrt(m) / DA_GAMMA * hbar;
    const double eta = pow(m, -DA_KAPPA);
    ad[AD_LOG_EPS_BAR] = eta * le + (1.0 - eta) * ad[AD_LOG_EPS_BAR];
    ad[AD_HBAR] = hbar;
    ad[AD_M] = m;
    ad[AD_EPS] = exp(le);
  }
}

// mode 1: (re)start the averaging at the current step size; mode 0: freeze the step size at the averaged one
__global__ void hmc_adapt_ctl_kernel(double *ad, int mode) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (mode == 1) {
    ad[AD_MU] = log(10.0 * ad[AD_EPS]);
    ad[AD_LOG_EPS_BAR] = 0.0;
    ad[AD_HBAR] = 0.0;
    ad[AD_M] = 0.0;
  } else if (ad[AD_M] > 0.0) {
    ad[AD_EPS] = exp(ad[AD_LOG_EPS_BAR]);
    ad[AD_M] = 0.0;
  }
}

// the raw draws of one step, for the tests of the random stream
__global__ __launch_bounds__(256) void hmc_draws_kernel(double *z, double *ua, double *uj, int W, int d, uint32_t k0,
                                                        uint32_t k1, uint32_t step_lo, uint32_t step_hi) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  const u32x4 r = philox4x32_10(u32x4{(uint32_t)w, 6u, step_lo, step_hi}, k0, k1);
  ua[w] = u01_from(r.x, r.y);
  uj[w] = u01_from(r.z, r.w);
  for (int j = 0; 2 * j < d; ++j) {
    double z0, z1;
    hmc_normal_pair((uint32_t)w, j, step_lo, step_hi, k0, k1, z0, z1);
    z[(int64_t)w * d + 2 * j] = z0;
    if (2 * j + 1 < d) z[(int64_t)w * d + 2 * j + 1] = z1;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static HmcArgs hmc_args(gpemu_sampler *s, int store_chain) {
  HmcState *h = s->hmc;
  const gpemu_model *m0 = s->groups[0];
  HmcArgs a;
  a.X = s->X; a.logp = s->logp; a.g = h->g;
  a.xq = h->xq; a.p = h->p; a.gnew = h->gnew; a.lpnew = h->lpnew;
  a.kin0 = h->kin0; a.epsw = h->epsw; a.logu = h->logu; a.accp = h->accp;
  a.minv = h->minv; a.lo = m0->lo; a.hi = m0->hi; a.ad = h->ad;
  a.naccept = s->naccept; a.ndiv = h->ndiv; a.flags = s->flags;
  a.chain = store_chain ? s->chain + s->chain_len * s->W * s->d : nullptr;
  a.lpchain = store_chain ? s->lpchain + s->chain_len * s->W : nullptr;
  a.W = (int)s->W; a.d = (int)s->d; a.dp = s->dp;
  return a;
}

static inline dim3 hmc_grid(const gpemu_sampler *s) { return dim3((unsigned)((s->W + 255) / 256)); }

// one iteration after the begin kernel: the L gradient evaluations and what lies between and after them
static int hmc_trajectory(gpemu_sampler *s, const HmcArgs &a, hipStream_t st) {
  HmcState *h = s->hmc;
  for (int l = 0; l < h->L; ++l) {
    GP_TRY(logpost_grad_eval(s->groups.data(), (int)s->groups.size(), s->W, h->xq, h->lpnew, h->gnew, st));
    if (l + 1 < h->L) {
      hipLaunchKernelGGL(hmc_leapfrog_kernel, hmc_grid(s), dim3(256), 0, st, a);
      hmc_path_count(GPEMU_HMC_PATH_LEAPFROG);
    }
  }
  hipLaunchKernelGGL(hmc_finish_kernel, hmc_grid(s), dim3(256), 0, st, a);
  hipLaunchKernelGGL(hmc_adapt_kernel, dim3(1), dim3(256), 0, st, h->accp, (int)s->W, h->ad, h->adapt_on, h->target);
  GP_HIP(hipGetLastError());
  hmc_path_count(GPEMU_HMC_PATH_FINISH);
  hmc_path_count(h->adapt_on ? GPEMU_HMC_PATH_ADAPT : GPEMU_HMC_PATH_ACCEPT_MEAN);
  if (a.chain) s->chain_len += 1;
  s->iterations += 1;
  s->step_counter += 1;
  return GPEMU_OK;
}

int hmc_run(gpemu_sampler *s, int64_t steps, int store_chain) {
  HmcState *h = s->hmc;
  hipStream_t st = s->stream;
  if (store_chain) GP_TRY(sampler_ensure_chain(s, s->chain_len + steps));
  const uint32_t k0 = (uint32_t)s->seed, k1 = (uint32_t)(s->seed >> 32);
  for (int64_t it = 0; it < steps; ++it) {
    const HmcArgs a = hmc_args(s, store_chain);
    const uint64_t step = s->step_counter;
    hipLaunchKernelGGL(hmc_begin_kernel<false>, hmc_grid(s), dim3(256), 0, st, a, k0, k1, (uint32_t)step,
                       (uint32_t)(step >> 32), h->jitter);
    hmc_path_count(GPEMU_HMC_PATH_BEGIN);
    GP_TRY(hmc_trajectory(s, a, st));
  }
  return sampler_check_nan(s);
}

// lp and the gradient of the current positions, through the gradient path (the lp every later accept compares with
// comes from that path as well)
int hmc_refresh_state(gpemu_sampler *s, const double *X, double *logp, hipStream_t st) {
  HmcState *h = s->hmc;
  GP_HIP(hipMemcpy2DAsync(h->xq, sizeof(double) * s->d, X, sizeof(double) * s->dp, sizeof(double) * s->d, (size_t)s->W,
                          hipMemcpyDeviceToDevice, st));
  GP_TRY(logpost_grad_eval(s->groups.data(), (int)s->groups.size(), s->W, h->xq, logp, h->g, st));
  return GPEMU_OK;
}

int hmc_reset(gpemu_sampler *s) {
  HmcState *h = s->hmc;
  GP_HIP(hipMemsetAsync(h->ndiv, 0, sizeof(long long) * s->W, s->stream));
  GP_HIP(hipMemsetAsync(h->ad + AD_LAST, 0, sizeof(double) * 3, s->stream));
  return GPEMU_OK;
}

int hmc_snapshot_reserve(gpemu_sampler *s) {
  HmcState *h = s->hmc;
  const int64_t W = s->W, d = s->d;
  if (!h->snapg) GP_TRY(dev_alloc(&h->snapg, W * d));
  if (!h->snapdiv) GP_TRY(dev_alloc(&h->snapdiv, W));
  if (!h->snapad) GP_TRY(dev_alloc(&h->snapad, AD_COUNT + HMC_MAX_D));
  return GPEMU_OK;
}

int hmc_snapshot(gpemu_sampler *s) {
  HmcState *h = s->hmc;
  const int64_t W = s->W, d = s->d;
  GP_HIP(hipMemcpyAsync(h->snapg, h->g, sizeof(double) * W * d, hipMemcpyDeviceToDevice, s->stream));
  GP_HIP(hipMemcpyAsync(h->snapdiv, h->ndiv, sizeof(long long) * W, hipMemcpyDeviceToDevice, s->stream));
  GP_HIP(hipMemcpyAsync(h->snapad, h->ad, sizeof(double) * AD_COUNT, hipMemcpyDeviceToDevice, s->stream));
  GP_HIP(hipMemcpyAsync(h->snapad + AD_COUNT, h->minv, sizeof(double) * HMC_MAX_D, hipMemcpyDeviceToDevice, s->stream));
  h->snap_adapt_on = h->adapt_on;
  h->snap_target = h->target;
  h->snap_minv = h->minv_host;
  return GPEMU_OK;
}

int hmc_restore(gpemu_sampler *s) {
  HmcState *h = s->hmc;
  const int64_t W = s->W, d = s->d;
  GP_HIP(hipMemcpyAsync(h->g, h->snapg, sizeof(double) * W * d, hipMemcpyDeviceToDevice, s->stream));
  GP_HIP(hipMemcpyAsync(h->ndiv, h->snapdiv, sizeof(long long) * W, hipMemcpyDeviceToDevice, s->stream));
  GP_HIP(hipMemcpyAsync(h->ad, h->snapad, sizeof(double) * AD_COUNT, hipMemcpyDeviceToDevice, s->stream));
  GP_HIP(hipMemcpyAsync(h->minv, h->snapad + AD_COUNT, sizeof(double) * HMC_MAX_D, hipMemcpyDeviceToDevice, s->stream));
  h->adapt_on = h->snap_adapt_on;
  h->target = h->snap_target;
  h->minv_host = h->snap_minv;
  return GPEMU_OK;
}

void hmc_release(gpemu_sampler *s) {
  HmcState *h = s->hmc;
  if (!h) return;
  dev_free(h->g); dev_free(h->xq); dev_free(h->p); dev_free(h->gnew); dev_free(h->lpnew); dev_free(h->kin0);
  dev_free(h->epsw); dev_free(h->logu); dev_free(h->accp); dev_free(h->minv); dev_free(h->ad); dev_free(h->ndiv);
  dev_free(h->snapg); dev_free(h->snapdiv); dev_free(h->snapad);
  delete h;
  s->hmc = nullptr;
}

static int hmc_fill(gpemu_sampler *s, double eps0) {
  HmcState *h = s->hmc;
  const int64_t W = s->W, d = s->d;
  GP_TRY(dev_alloc(&h->g, W * d));
  GP_TRY(dev_alloc(&h->xq, W * d));
  GP_TRY(dev_alloc(&h->p, W * d));
  GP_TRY(dev_alloc(&h->gnew, W * d));
  GP_TRY(dev_alloc(&h->lpnew, W));
  GP_TRY(dev_alloc(&h->kin0, W));
  GP_TRY(dev_alloc(&h->epsw, W));
  GP_TRY(dev_alloc(&h->logu, W));
  GP_TRY(dev_alloc(&h->accp, W));
  GP_TRY(dev_alloc(&h->minv, HMC_MAX_D));
  GP_TRY(dev_alloc(&h->ad, AD_COUNT));
  GP_TRY(dev_alloc(&h->ndiv, W));
  const gpemu_model *m0 = s->groups[0];
  std::vector<double> lo(m0->dp), hi(m0->dp);
  GP_HIP(hipMemcpy(lo.data(), m0->lo, sizeof(double) * m0->dp, hipMemcpyDeviceToHost));
  GP_HIP(hipMemcpy(hi.data(), m0->hi, sizeof(double) * m0->dp, hipMemcpyDeviceToHost));
  h->minv_host.assign(HMC_MAX_D, 1.0);
  for (int64_t i = 0; i < d; ++i) h->minv_host[i] = (hi[i] - lo[i]) * (hi[i] - lo[i]) / 12.0;
  double ad[AD_COUNT] = {0.0};
  ad[AD_EPS] = eps0;
  ad[AD_MU] = std::log(10.0 * eps0);
  GP_HIP(hipMemcpy(h->minv, h->minv_host.data(), sizeof(double) * HMC_MAX_D, hipMemcpyHostToDevice));
  GP_HIP(hipMemcpy(h->ad, ad, sizeof(double) * AD_COUNT, hipMemcpyHostToDevice));
  GP_HIP(hipMemset(h->g, 0, sizeof(double) * W * d));
  GP_HIP(hipMemset(h->ndiv, 0, sizeof(long long) * W));
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

#define GP_HMC(s, name)                                                                         \
  do {                                                                                          \
    GP_ARG(s, "sampler");                                                                       \
    if (!(s)->hmc) { set_error(name ": the sampler is not an HMC sampler"); return GPEMU_ERR_STATE; } \
  } while (0)

extern "C" {

int gpemu_sampler_create_hmc(gpemu_sampler **out, gpemu_model *const *groups, int n_groups, int64_t W, int n_leapfrog,
                             double eps0, double jitter, uint64_t seed) {
  GP_ARG(out && groups && n_groups > 0, "groups");
  *out = nullptr;
  GP_ARG(n_leapfrog >= 1 && n_leapfrog <= 4096, "n_leapfrog must be in [1, 4096]");
  GP_ARG(eps0 > 0.0 && std::isfinite(eps0), "the step size must be positive and finite");
  GP_ARG(jitter >= 0.0 && jitter < 1.0, "jitter must be in [0, 1)");
  for (int g = 0; g < n_groups; ++g) {
    GP_ARG(groups[g], "null group");
    GP_TRY(grad_lik_supported(groups[g], "hmc sampler"));     // whatever the gradient declines, before any launch
  }
  gpemu_sampler *s = nullptr;
  GP_TRY(gpemu_sampler_create_chains(&s, groups, n_groups, W, 2.0, &seed, 1));
  s->hmc = new HmcState();
  s->hmc->L = n_leapfrog;
  s->hmc->jitter = jitter;
  const int rc = hmc_fill(s, eps0);
  if (rc != GPEMU_OK) {
    gpemu_sampler_destroy(s);
    return rc;
  }
  *out = s;
  return GPEMU_OK;
}

int gpemu_sampler_hmc_set_metric(gpemu_sampler *s, const double *minv) {
  GP_HMC(s, "gpemu_sampler_hmc_set_metric");
  GP_ARG(minv, "minv");
  for (int64_t i = 0; i < s->d; ++i) GP_ARG(minv[i] > 0.0 && std::isfinite(minv[i]), "the inverse metric must be positive and finite");
  GP_HIP(hipSetDevice(s->device));
  HmcState *h = s->hmc;
  GP_HIP(hipStreamSynchronize(s->stream));
  for (int64_t i = 0; i < s->d; ++i) h->minv_host[i] = minv[i];
  GP_HIP(hipMemcpy(h->minv, h->minv_host.data(), sizeof(double) * HMC_MAX_D, hipMemcpyHostToDevice));
  return GPEMU_OK;
}

int gpemu_sampler_hmc_get_metric(gpemu_sampler *s, double *minv) {
  GP_HMC(s, "gpemu_sampler_hmc_get_metric");
  GP_ARG(minv, "minv");
  for (int64_t i = 0; i < s->d; ++i) minv[i] = s->hmc->minv_host[i];
  return GPEMU_OK;
}

int gpemu_sampler_hmc_set_step_size(gpemu_sampler *s, double eps) {
  GP_HMC(s, "gpemu_sampler_hmc_set_step_size");
  GP_ARG(eps > 0.0 && std::isfinite(eps), "the step size must be positive and finite");
  GP_HIP(hipSetDevice(s->device));
  GP_HIP(hipStreamSynchronize(s->stream));
  GP_HIP(hipMemcpy(s->hmc->ad + AD_EPS, &eps, sizeof(double), hipMemcpyHostToDevice));
  if (s->hmc->adapt_on) hipLaunchKernelGGL(hmc_adapt_ctl_kernel, dim3(1), dim3(64), 0, s->stream, s->hmc->ad, 1);
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

int gpemu_sampler_hmc_get_step_size(gpemu_sampler *s, double *eps) {
  GP_HMC(s, "gpemu_sampler_hmc_get_step_size");
  GP_ARG(eps, "eps");
  GP_HIP(hipSetDevice(s->device));
  GP_HIP(hipMemcpyAsync(eps, s->hmc->ad + AD_EPS, sizeof(double), hipMemcpyDeviceToHost, s->stream));
  GP_HIP(hipStreamSynchronize(s->stream));
  return GPEMU_OK;
}

int gpemu_sampler_hmc_adapt(gpemu_sampler *s, int on, double target_accept) {
  GP_HMC(s, "gpemu_sampler_hmc_adapt");
  GP_ARG(!on || (target_accept > 0.0 && target_accept < 1.0), "target_accept must be in (0, 1)");
  GP_HIP(hipSetDevice(s->device));
  HmcState *h = s->hmc;
  // on: the averaging (re)starts at the current step size; off after on: the step size freezes at the averaged one
  if (on || h->adapt_on) hipLaunchKernelGGL(hmc_adapt_ctl_kernel, dim3(1), dim3(64), 0, s->stream, h->ad, on ? 1 : 0);
  GP_HIP(hipGetLastError());
  h->adapt_on = on ? 1 : 0;
  if (on) h->target = target_accept;
  return GPEMU_OK;
}

int gpemu_sampler_hmc_step_host_rng(gpemu_sampler *s, const double *p0, const double *logu, const double *eps_w,
                                    int store_chain) {
  GP_HMC(s, "gpemu_sampler_hmc_step_host_rng");
  GP_ARG(p0 && logu && eps_w, "null pointer");
  GP_HIP(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  HmcState *h = s->hmc;
  if (store_chain) GP_TRY(sampler_ensure_chain(s, s->chain_len + 1));
  GP_TRY(upload(h->p, p0, s->W * s->d, st));
  GP_TRY(upload(h->logu, logu, s->W, st));
  GP_TRY(upload(h->epsw, eps_w, s->W, st));
  const HmcArgs a = hmc_args(s, store_chain);
  hipLaunchKernelGGL(hmc_begin_kernel<true>, hmc_grid(s), dim3(256), 0, st, a, 0u, 0u, 0u, 0u, 0.0);
  hmc_path_count(GPEMU_HMC_PATH_BEGIN_HOST_RNG);
  GP_TRY(hmc_trajectory(s, a, st));
  return sampler_check_nan(s);   // also synchronises: the caller's arrays are free again
}

int gpemu_sampler_hmc_stats(gpemu_sampler *s, int64_t *naccepted, int64_t *divergences, double *mean_accept_prob,
                            double *last_accept_prob) {
  GP_HMC(s, "gpemu_sampler_hmc_stats");
  GP_HIP(hipSetDevice(s->device));
  double ad[AD_COUNT];
  if (naccepted) GP_HIP(hipMemcpyAsync(naccepted, s->naccept, sizeof(long long) * s->W, hipMemcpyDeviceToHost, s->stream));
  if (divergences) GP_HIP(hipMemcpyAsync(divergences, s->hmc->ndiv, sizeof(long long) * s->W, hipMemcpyDeviceToHost, s->stream));
  GP_HIP(hipMemcpyAsync(ad, s->hmc->ad, sizeof(double) * AD_COUNT, hipMemcpyDeviceToHost, s->stream));
  GP_HIP(hipStreamSynchronize(s->stream));
  if (mean_accept_prob) *mean_accept_prob = ad[AD_N] > 0.0 ? ad[AD_SUM] / ad[AD_N] : 0.0;
  if (last_accept_prob) *last_accept_prob = ad[AD_LAST];
  return GPEMU_OK;
}

int gpemu_sampler_hmc_draws(gpemu_sampler *s, uint64_t step, double *z, double *u_accept, double *u_jitter) {
  GP_HMC(s, "gpemu_sampler_hmc_draws");
  GP_ARG(z && u_accept && u_jitter, "null pointer");
  GP_HIP(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const int64_t W = s->W, d = s->d;
  DevScope sc(st);
  double *dz, *du;
  GP_TRY(sc.alloc(&dz, W * d));
  GP_TRY(sc.alloc(&du, 2 * W));
  hipLaunchKernelGGL(hmc_draws_kernel, hmc_grid(s), dim3(256), 0, st, dz, du, du + W, (int)W, (int)d, (uint32_t)s->seed,
                     (uint32_t)(s->seed >> 32), (uint32_t)step, (uint32_t)(step >> 32));
  GP_HIP(hipGetLastError());
  GP_TRY(sc.download(z, dz, W * d));
  GP_TRY(sc.download(u_accept, du, W));
  GP_TRY(sc.download(u_jitter, du + W, W));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_sampler_chain_moments(gpemu_sampler *s, int64_t first, int64_t n, double *mean, double *var) {
  GP_ARG(s && mean && var, "null pointer");
  GP_ARG(first >= 0 && n >= 1 && first + n <= s->chain_len, "chain range");
  GP_HIP(hipSetDevice(s->device));
  GP_TRY(moments_to_host(s->chain + first * s->W * s->d, n * s->W, (int)s->d, mean, var, s->stream));
  hmc_path_count(GPEMU_HMC_PATH_MOMENTS);
  return GPEMU_OK;
}

int gpemu_hmc_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_HMC, out, n); }

}  // extern "C"
