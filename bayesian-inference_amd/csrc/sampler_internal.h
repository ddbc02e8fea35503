// Sampler state shared by k_sampler.hip (stretch move, phase API, RCCL run), k_front.hip (fused run), k_temper.hip
// (parallel tempering), k_hmc.hip (Hamiltonian Monte Carlo), k_acf.hip (autocorrelation) and the summaries of the stored
// chain: k_postpred.hip, k_diag.hip, k_marginal.hip, k_reweight.hip and what they share, k_rows.hip and k_select.hip
// (rows_dev.h).
#pragma once
#include <vector>

#include "internal.h"

namespace gpemu {
constexpr int RNG_RING = 32;        // steps of randomness kept on the device
constexpr int RNG_BATCH = 16;       // steps generated per launch (half the ring: the previous step's draws stay
                                    // readable while the next batch is written)
constexpr int GATHER_SLOTS = 3;
// a log-probability that has not arrived yet: a quiet NaN with a payload no computation produces
constexpr unsigned long long GATHER_EMPTY = 0x7FF8DEADBEEF0001ull;

// ---- Philox4x32-10 (Salmon et al., SC'11) ----------------------------------------------------
struct u32x4 { uint32_t x, y, z, w; };
__host__ __device__ static inline u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)M0 * c.x, p1 = (uint64_t)M1 * c.z;
    u32x4 n;
    n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
    n.y = (uint32_t)p1;
    n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
    n.w = (uint32_t)p0;
    c = n;
    k0 += W0;
    k1 += W1;
  }
  return c;
}
__host__ __device__ static inline double u01_from(uint32_t hi, uint32_t lo) {
  uint64_t v = ((uint64_t)hi << 32) | lo;
  return (double)(v >> 11) * (1.0 / 9007199254740992.0);  // [0,1), 53 bits
}
}  // namespace gpemu

// what an HMC sampler (gpemu_sampler_create_hmc, k_hmc.hip) holds beside the chain layout of gpemu_sampler
struct HmcState {
  int L = 1;                   // leapfrog steps per iteration
  double jitter = 0.0;         // eps_w = eps (1 + jitter (2 u - 1))
  int adapt_on = 0;            // dual averaging of the step size after every iteration
  double target = 0.8;         // its target mean accept probability
  double *g = nullptr;         // [W][d]  gradient of the current state, carried between the iterations
  double *xq = nullptr;        // [W][d]  trajectory position (unpadded rows: the gradient path's input)
  double *p = nullptr;         // [W][d]  trajectory momentum
  double *gnew = nullptr;      // [W][d]  gradient at xq
  double *lpnew = nullptr;     // [W]     log-posterior at xq
  double *kin0 = nullptr;      // [W]     kinetic energy of the drawn momentum
  double *epsw = nullptr;      // [W]     the chains' step sizes of this iteration
  double *logu = nullptr;      // [W]     log of the accept uniform
  double *accp = nullptr;      // [W]     min(1, exp(H_old - H_new)), 0 for a divergence
  double *minv = nullptr;      // [16]    diagonal inverse metric (1 beyond d)
  double *ad = nullptr;        // step size and dual-averaging state (k_hmc.hip: AD_*)
  long long *ndiv = nullptr;   // [W]     divergences
  std::vector<double> minv_host;
  // gpemu_sampler_snapshot / _restore
  double *snapg = nullptr, *snapad = nullptr;
  long long *snapdiv = nullptr;
  int snap_adapt_on = 0;
  double snap_target = 0.8;
  std::vector<double> snap_minv;
};

struct gpemu_sampler {
  HmcState *hmc = nullptr;     // an HMC sampler: the stretch move's fields below are allocated but idle
  int device = 0;
  std::vector<gpemu_model *> groups;
  int64_t W = 0, d = 0;
  int dp = gpemu::DPAD;        // padded width of X, Xbuf, q, q2, snapX: dpad_of(d) (the groups' dp)
  int64_t ns[2] = {0, 0};      // set sizes: ceil(W/2), floor(W/2)
  int64_t qcap = 0;            // rows of q (>= ns[0] rounded up to 128, + 128)
  double a = 2.0;
  uint64_t seed = 0;
  int nchains = 1;             // independent chains stacked in this sampler (W = nchains x walkers per chain)
  unsigned long long *seeds = nullptr;   // [nchains] Philox keys, on the device
  uint64_t step_counter = 0;   // RNG counter, never reset
  int64_t iterations = 0;      // steps since the last reset
  hipStream_t stream = nullptr;
  double *X = nullptr;         // [W][dp]  current positions: one of the two halves of Xbuf
  double *logp = nullptr;      // [W]        current log-probabilities: one of the two halves of lpbuf
  double *Xbuf = nullptr;      // [2][W][dp]  the fused run writes the accepted state into the other half
  double *lpbuf = nullptr;     // [2][W]
  int cur = 0;                 // which half X / logp point at
  // per-step randomness, ring of RNG_RING steps (slot = step_counter % RNG_RING)
  int *inds = nullptr;         // [RING][W] split of each walker
  int *idx = nullptr;          // [RING][2][W] members of each set, ascending walker index
  double *zz = nullptr;        // [RING][2][W]
  double *logu = nullptr;      // [RING][2][W]
  int *rint = nullptr;         // [RING][2][W]  partner walker of each proposal: c[randint(nc)] as a walker index
  double *fac = nullptr;       // [RING][2][W]  (d - 1) log zz
  int *pos = nullptr;          // [RING][W]     position of each walker in its set's list
  uint64_t rng_ready_until = 0; // steps [.., rng_ready_until) of the device stream are in the ring
  double *q = nullptr;         // [qcap][dp]
  double *factors = nullptr;   // [W]
  double *newlp = nullptr;     // [qcap]
  long long *naccept = nullptr;  // [W]
  int *flags = nullptr;        // [1] count of NaN log-probabilities seen
  // compacted half-step (k_sampler.hip: propose_compact_kernel): the proposals inside the prior box, in their order, are
  // rows 0 .. *n_live - 1 of q, and only they are evaluated
  int *slot_of = nullptr;      // [qcap] row of proposal i of the chunk in flight, -1 outside the box
  int *n_live = nullptr;       // [1]    rows of q that hold proposals
  long long *live_cnt = nullptr;   // [2] proposals inside the box / proposals, over every compacted chunk so far
  double *chain = nullptr;     // [chain_cap][W][d]
  double *lpchain = nullptr;   // [chain_cap][W]
  int64_t chain_cap = 0, chain_len = 0;
  uint64_t chain_epoch = 0;    // bumped by whatever may move or rewrite the stored chain (a storing run, reserve, reset,
                               // restore): a gpemu_diag that borrowed the chain before is stale (k_diag.hip)
  // multi-GPU: this rank's slice / the gathered log-probabilities of each half ([per] / [per*world])
  double *gmine[2] = {nullptr, nullptr};
  double *gfull[2] = {nullptr, nullptr};
  int64_t gper[2] = {0, 0};
  int gworld = 0;
  // fused run (k_front.hip): proposals of the half in flight and of the one before, log-probability exchange
  double *q2 = nullptr;        // [2][qcap][dp]
  double *gather = nullptr;    // [GATHER_SLOTS][ns[0]]  this rank's copy of every proposal's new log-probability
  bool gather_uncached = false;
  double **peers = nullptr;    // device array [peer_world]: every rank's gather buffer (own one included)
  std::vector<void *> peer_opened;   // IPC mappings to close
  int peer_world = 0, peer_rank = 0;
  int device_share = 1;        // ranks of the job whose samplers run on this device (gpemu_sampler_peer_share)
  uint64_t front_count = 0;    // fused launches so far (gather slot and buffer parity)
  // XCD-aware order of the front kernel's cross-kernel workgroups, per (share size, group): device tables (k_front.hip)
  struct FrontPerm { int64_t cnt; int group, wg0; int *dperm; };
  std::vector<FrontPerm> front_perms;
  // snapshot of the chain state (gpemu_sampler_snapshot / _restore): a block of steps that failed -- a lost peer
  // exchange -- is rerun from here over another transport and gives the chain of an unbroken run
  double *snapX = nullptr, *snaplp = nullptr;        // [W][dp], [W]
  long long *snapacc = nullptr;                      // [W]
  long long *snapswap = nullptr;                     // tempered: [2][nchains - 1][W / nchains] swap counters
  bool snap_valid = false;
  uint64_t snap_step_counter = 0;
  int64_t snap_iterations = 0, snap_chain_len = 0;
  // autocorrelation estimate (k_acf.hip): scratch kept between the lag blocks of one estimate
  double *acf_part = nullptr, *acf_acf = nullptr, *acf_mean = nullptr, *acf_acf0 = nullptr;
  size_t acf_part_bytes = 0, acf_acf_bytes = 0, acf_mean_bytes = 0;   // capacity of acf_part / acf_acf / acf_mean + acf_acf0
  int64_t acf_first = -1, acf_n = -1, acf_w0 = -1, acf_nw = -1;       // the estimate the scratch belongs to
  uint64_t acf_epoch = 0;            // chain_epoch at that estimate's first block: a later block under another is refused
  // parallel tempering (gpemu_sampler_create_tempered, k_temper.hip): the nchains stacked chains are the rungs of a
  // temperature ladder on ONE data vector; rung t accepts with beta[t] and swaps states with rung t - 1 every
  // swap_every steps
  bool tempered = false;
  int swap_every = 0;                // 0: no swaps
  double *betas = nullptr;           // [nchains] inverse temperatures, betas[0] = 1 >= betas[1] >= ... >= 0
  long long *nswap_acc = nullptr;    // [nchains - 1][W / nchains] accepted swaps of rung pair (t, t + 1), column w
  long long *nswap_try = nullptr;    // [nchains - 1][W / nchains] attempted swaps
  double *mean_ll = nullptr;         // [nchains] scratch of gpemu_sampler_mean_loglik
};

namespace gpemu {
// order-preserving 64-bit key of a double (negative: all bits flipped, else the sign bit set) and its inverse: the
// radix select (k_select.hip) and the radix sort (k_rows.hip)
typedef unsigned long long u64;
static __device__ __forceinline__ u64 sel_key(double v) {
  const u64 u = (u64)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
static __device__ __forceinline__ double sel_value(u64 key) {
  const u64 u = (key >> 63) ? (key ^ 0x8000000000000000ull) : ~key;
  return __longlong_as_double((long long)u);
}
// what a summary returns where no element answers: the quiet NaN
static __device__ __forceinline__ double sel_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
// k_acf.hip: per-series sums, means and lag products of a block of series (the kernels' own comments), which
// k_diag.hip runs on the transformed split chains
__global__ __launch_bounds__(256) void acf_sum_kernel(const double *__restrict__ chain, int64_t n_t, int64_t S, int64_t ld, int64_t tchunk,
                               double *__restrict__ part);
__global__ __launch_bounds__(256) void acf_mean_kernel(const double *__restrict__ part, int64_t n_t, int64_t S, int nchunk,
                                double *__restrict__ mean);
__global__ __launch_bounds__(256) void acf_lag_kernel(const double *__restrict__ chain, const double *__restrict__ mean, int64_t n_t, int64_t S,
                               int64_t ld, int64_t tchunk, int64_t lag0, int n_lags, double *__restrict__ part);
__global__ __launch_bounds__(256) void acf_reduce_kernel(const double *__restrict__ part, int64_t S, int n_lags, int nchunk,
                                  double *__restrict__ acf, double *__restrict__ acf0, int is_first);
constexpr int ACF_LPT = 16;      // lags per thread
constexpr int ACF_TCHUNKS = 8;   // chunks of steps (partial sums)
// k_sampler.hip
int sampler_launch_rng(gpemu_sampler *s, hipStream_t st, int64_t ahead);
int sampler_ensure_chain(gpemu_sampler *s, int64_t need);
int sampler_check_nan(gpemu_sampler *s);
// k_temper.hip
int temper_swap(gpemu_sampler *s, int store_chain, hipStream_t st);   // the swap pass of step s->step_counter, if due
int temper_validate_ladder(const double *betas, int n_temps);
// k_hmc.hip: the parts of the sampler calls that an HMC sampler (s->hmc) takes
int hmc_run(gpemu_sampler *s, int64_t steps, int store_chain);
// lp (into logp) and the gradient of the padded positions X [W][dp] that gpemu_sampler_set_state is about to make current
int hmc_refresh_state(gpemu_sampler *s, const double *X, double *logp, hipStream_t st);
int hmc_reset(gpemu_sampler *s);
int hmc_snapshot_reserve(gpemu_sampler *s);   // the snapshot's buffers, before anything of it is written
int hmc_snapshot(gpemu_sampler *s);
int hmc_restore(gpemu_sampler *s);
void hmc_release(gpemu_sampler *s);
// the calls an HMC sampler declines
#define GP_NOT_HMC(s, name)                                                                              \
  do {                                                                                                   \
    if ((s) && (s)->hmc) {                                                                               \
      gpemu::set_error(name ": not supported on an HMC sampler (one GPU, gpemu_sampler_run)");           \
      return GPEMU_ERR_UNSUPPORTED;                                                                      \
    }                                                                                                    \
  } while (0)
// k_front.hip
void front_release(gpemu_sampler *s);                         // frees the gather buffer and the peer mappings
bool front_eligible(const gpemu_sampler *s);
bool front_eligible_for(const gpemu_sampler *s, int world);   // ... and, with several ranks on this device, their launches fit on it together
// `steps` stretch-move steps with two launches per half-step (fused front kernel + triangular GEMM); world / rank:
// how the proposing half is split (world = 1: everything here); emulate: evaluate rank 0's share of a `world`-rank job
int front_run(gpemu_sampler *s, int64_t steps, int store_chain, int world, int rank, bool emulate);
}  // namespace gpemu
