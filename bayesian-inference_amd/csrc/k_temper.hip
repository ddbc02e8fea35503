// Parallel tempering on the stacked-chain sampler.
//
// A tempered sampler is a stacked sampler (gpemu_sampler_create_chains) whose T chains -- the rungs of a temperature
// ladder betas[0] = 1 >= betas[1] >= ... >= betas[T-1] >= 0 -- share ONE data vector.  Rung t owns walkers
// t Wc .. t Wc + Wc - 1, draws its stretch moves from its own key seeds[t] exactly as a one-chain sampler does, and
// accepts with the log-likelihood difference scaled by betas[t] (tempered_accept, internal.h: the accept kernels).
// After step s, when (s + 1) % swap_every == 0, the swap pass below walks the ladder from hot to cold for every walker
// column w: rung t's walker w and rung t-1's walker w exchange states with probability
//     min(1, exp((betas[t-1] - betas[t]) (ll[t][w] - ll[t-1][w]))),
// the uniform from Philox(c = (w, 5, s_lo, s_hi), key = seeds[t]) (streams 0 .. 4 are the stretch draws).  The stored
// log-probabilities are the untempered ll; mean_ll_kernel averages them per rung for the thermodynamic-integration
// evidence (gpemu/tempering.py).
#include "internal.h"
#include "sampler_internal.h"
#include "wg_dev.h"

#include <algorithm>
#include <cmath>

namespace gpemu {

// One thread per walker column; the ladder is walked serially (a swap of (t, t-1) sees the state the swap of
// (t+1, t) left).  Exchanges full padded rows of X, the log-probabilities and -- if the step is recorded -- the chain
// row the accept kernels wrote for this step.  No atomics: column w's counters are this thread's alone.
template <int DP>
__global__ __launch_bounds__(256) void temper_swap_kernel(double *__restrict__ X, double *__restrict__ logp,
                                                          double *__restrict__ chain, double *__restrict__ lpchain,
                                                          const double *__restrict__ betas,
                                                          const unsigned long long *__restrict__ seeds,
                                                          long long *__restrict__ nacc, long long *__restrict__ ntry,
                                                          int T, int Wc, int d, unsigned long long step) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= Wc) return;
  const uint32_t step_lo = (uint32_t)step, step_hi = (uint32_t)(step >> 32);
  for (int t = T - 1; t >= 1; --t) {
    const int64_t hot = (int64_t)t * Wc + w, cold = (int64_t)(t - 1) * Wc + w;
    const unsigned long long key = seeds[t];
    const u32x4 r = philox4x32_10(u32x4{(uint32_t)w, 5u, step_lo, step_hi}, (uint32_t)key, (uint32_t)(key >> 32));
    const double logu = log(u01_from(r.x, r.y));
    const double lh = logp[hot], lc = logp[cold];
    const int64_t slot = (int64_t)(t - 1) * Wc + w;
    ntry[slot] += 1;
    if (!(__builtin_isfinite(lh) && __builtin_isfinite(lc))) continue;
    if (!(logu < (betas[t - 1] - betas[t]) * (lh - lc))) continue;
    nacc[slot] += 1;
    logp[hot] = lc;
    logp[cold] = lh;
#pragma unroll
    for (int dd = 0; dd < DP; ++dd) {
      const double a = X[hot * DP + dd], b = X[cold * DP + dd];
      X[hot * DP + dd] = b;
      X[cold * DP + dd] = a;
    }
    if (chain) {
      for (int dd = 0; dd < d; ++dd) {
        const double a = chain[hot * d + dd], b = chain[cold * d + dd];
        chain[hot * d + dd] = b;
        chain[cold * d + dd] = a;
      }
      lpchain[hot] = lc;
      lpchain[cold] = lh;
    }
  }
}

// mean_ll[t] = mean of lpchain[first .. first + n)[t Wc .. t Wc + Wc): one workgroup per rung.  Every thread adds a
// fixed strided set of entries in a fixed order, then tree A of wg_dev.h over the 1024 threads: the same bits on every
// run.
constexpr int MEAN_LL_THREADS = 1024;
__global__ __launch_bounds__(MEAN_LL_THREADS) void mean_ll_kernel(const double *__restrict__ lpchain, double *__restrict__ out,
                                                                  int64_t first, int64_t n, int Wc, int64_t W) {
  __shared__ double part[MEAN_LL_THREADS];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t total = n * Wc;
  double acc = 0.0;
  for (int64_t i = tid; i < total; i += MEAN_LL_THREADS) {
    const int64_t row = first + i / Wc, w = i % Wc;
    acc += lpchain[row * W + (int64_t)t * Wc + w];
  }
  acc = wg_sum_a<MEAN_LL_THREADS>(acc, part);
  if (tid == 0) out[t] = acc / (double)total;
}

int temper_validate_ladder(const double *betas, int n_temps) {
  GP_ARG(betas, "betas");
  GP_ARG(n_temps >= 2 && n_temps <= 64, "n_temps must be in [2, 64]");
  GP_ARG(betas[0] == 1.0, "betas[0] must be 1");
  for (int t = 1; t < n_temps; ++t) {
    GP_ARG(betas[t] >= 0.0 && betas[t] <= 1.0, "betas must lie in [0, 1]");
    GP_ARG(betas[t] <= betas[t - 1], "betas must be non-increasing");
  }
  return GPEMU_OK;
}

int temper_swap(gpemu_sampler *s, int store_chain, hipStream_t st) {
  if (s->swap_every <= 0 || (s->step_counter + 1) % (uint64_t)s->swap_every != 0) return GPEMU_OK;
  const int T = s->nchains, Wc = (int)(s->W / T);
  double *chain = nullptr, *lpchain = nullptr;
  if (store_chain) {         // the row of this step (end_step has not advanced chain_len yet)
    chain = s->chain + s->chain_len * s->W * s->d;
    lpchain = s->lpchain + s->chain_len * s->W;
  }
  hipLaunchKernelGGL(s->dp == DPAD ? temper_swap_kernel<DPAD> : temper_swap_kernel<DPAD_WIDE>, dim3((Wc + 255) / 256),
                     dim3(256), 0, st, s->X, s->logp, chain, lpchain, s->betas, s->seeds, s->nswap_acc, s->nswap_try,
                     T, Wc, (int)s->d, (unsigned long long)s->step_counter);
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;
extern "C" {

int gpemu_sampler_create_tempered(gpemu_sampler **out, gpemu_model *const *groups, int n_groups, int64_t Wc, double a,
                                  const uint64_t *seeds, const double *betas, int n_temps, int swap_every) {
  GP_ARG(out && groups && n_groups > 0 && seeds, "groups / seeds");
  *out = nullptr;
  GP_TRY(temper_validate_ladder(betas, n_temps));
  GP_ARG(swap_every >= 0, "swap_every must be >= 0");
  for (int g = 0; g < n_groups; ++g) {
    GP_ARG(groups[g], "null group");
    if (groups[g]->lik_ready && groups[g]->lik_chains != 1) {
      set_error("group %d carries %d data vectors: the rungs of a tempered sampler share one", g, groups[g]->lik_chains);
      return GPEMU_ERR_STATE;
    }
  }
  gpemu_sampler *s = nullptr;
  GP_TRY(gpemu_sampler_create_chains(&s, groups, n_groups, Wc, a, seeds, n_temps));
  const size_t npair = (size_t)(n_temps - 1) * (size_t)Wc;
  const int rc = [&]() -> int {     // the ladder's fields: the sampler is destroyed if one of them fails
    GP_TRY(dev_alloc(&s->betas, n_temps));
    GP_TRY(dev_alloc(&s->nswap_acc, (int64_t)npair));
    GP_TRY(dev_alloc(&s->nswap_try, (int64_t)npair));
    GP_TRY(dev_alloc(&s->mean_ll, n_temps));
    GP_HIP(hipMemcpy(s->betas, betas, sizeof(double) * n_temps, hipMemcpyHostToDevice));
    GP_HIP(hipMemsetAsync(s->nswap_acc, 0, sizeof(long long) * npair, s->stream));
    GP_HIP(hipMemsetAsync(s->nswap_try, 0, sizeof(long long) * npair, s->stream));
    GP_HIP(hipStreamSynchronize(s->stream));
    return GPEMU_OK;
  }();
  if (rc != GPEMU_OK) {
    gpemu_sampler_destroy(s);
    return rc;
  }
  s->tempered = true;
  s->swap_every = swap_every;
  *out = s;
  return GPEMU_OK;
}

int gpemu_sampler_set_betas(gpemu_sampler *s, const double *betas) {
  GP_ARG(s, "sampler");
  GP_NOT_HMC(s, "gpemu_sampler_set_betas");
  if (!s->tempered) { set_error("gpemu_sampler_set_betas: the sampler is not tempered"); return GPEMU_ERR_STATE; }
  GP_TRY(temper_validate_ladder(betas, s->nchains));
  GP_HIP(hipSetDevice(s->device));
  GP_HIP(hipStreamSynchronize(s->stream));    // launches in flight read the old ladder
  GP_HIP(hipMemcpy(s->betas, betas, sizeof(double) * s->nchains, hipMemcpyHostToDevice));
  return GPEMU_OK;
}

int gpemu_sampler_get_swap_counts(gpemu_sampler *s, int64_t *accepted, int64_t *attempted) {
  GP_ARG(s, "sampler");
  GP_NOT_HMC(s, "gpemu_sampler_get_swap_counts");
  if (!s->tempered) { set_error("gpemu_sampler_get_swap_counts: the sampler is not tempered"); return GPEMU_ERR_STATE; }
  GP_HIP(hipSetDevice(s->device));
  const size_t npair = (size_t)(s->nchains - 1) * (size_t)(s->W / s->nchains);
  if (accepted) GP_HIP(hipMemcpyAsync(accepted, s->nswap_acc, sizeof(long long) * npair, hipMemcpyDeviceToHost, s->stream));
  if (attempted) GP_HIP(hipMemcpyAsync(attempted, s->nswap_try, sizeof(long long) * npair, hipMemcpyDeviceToHost, s->stream));
  GP_HIP(hipStreamSynchronize(s->stream));
  return GPEMU_OK;
}

int gpemu_sampler_mean_loglik(gpemu_sampler *s, int64_t first, int64_t n, double *out) {
  GP_ARG(s && out, "sampler / out");
  GP_NOT_HMC(s, "gpemu_sampler_mean_loglik");
  if (!s->tempered) { set_error("gpemu_sampler_mean_loglik: the sampler is not tempered"); return GPEMU_ERR_STATE; }
  GP_ARG(first >= 0 && n >= 1 && first + n <= s->chain_len, "chain range");
  GP_HIP(hipSetDevice(s->device));
  const int T = s->nchains;
  hipLaunchKernelGGL(mean_ll_kernel, dim3(T), dim3(MEAN_LL_THREADS), 0, s->stream, s->lpchain, s->mean_ll, first, n,
                     (int)(s->W / T), s->W);
  GP_HIP(hipGetLastError());
  GP_HIP(hipMemcpyAsync(out, s->mean_ll, sizeof(double) * T, hipMemcpyDeviceToHost, s->stream));
  GP_HIP(hipStreamSynchronize(s->stream));
  return GPEMU_OK;
}

}  // extern "C"
