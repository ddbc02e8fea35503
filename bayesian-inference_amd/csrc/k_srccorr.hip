// Fully correlated systematic sources in the low-rank likelihood.
//
// The data covariance over all groups' features is  C_d = blockdiag_o(C_o) + B B^T,  B = [b_0 .. b_{S-1}] (S <= 16),
// so the likelihood's covariance is  Sigma = Sigma_bd + B B^T,  Sigma_bd = blockdiag over (group, observable block) of
// Sigma_o = A_o + U_o D U_o^T (k_loglik.hip; A_o carries C_o).  Woodbury and the matrix-determinant lemma give
//     log p = log p_bd + 1/2 ||L_K^-1 c||^2 - sum log diag L_K,
//     c = sum_o B_o^T Sigma_o^-1 r_o,   K = I_S + sum_o B_o^T Sigma_o^-1 B_o = L_K L_K^T,
// where log p_bd is the block-diagonal sum the likelihood launches already wrote.  With the setup's constants
// W_o = U_o^T A_o^-1 B_o, Q_o = B_o^T A_o^-1 B_o, w0_o = B_o^T A_o^-1 r0_o and, per walker, the block's
// M_o = I + D^1/2 G_o D^1/2 = L L^T and y_o = L^-1 D^1/2 (G_o m + g0_o):
//     T_o = L^-1 D^1/2 W_o,   c_o = W_o^T m + w0_o - T_o^T y_o,   Z_o = Q_o - T_o^T T_o.
//
// One workgroup per proposal, four waves; wave w takes the (group, block) tasks w, w + 4, ... in turn (lane = PC index,
// as loglik_dev.h) and refactors the block's M_o in LDS with the likelihood's own pieces (loglik_dev.h: lowrank_fill_lds,
// wave_cholesky_lds), adding its c_o and Z_o to accumulators of its own.  After one
// barrier wave 0 adds the four waves' accumulators in wave order (the same bits on every run), factors K (lane = row)
// and finishes the stretch move of the proposal's walker (loglik_dev.h: finish_walker).  No workgroup waits for another.
#include <algorithm>

#include "internal.h"
#include "loglik_dev.h"

namespace gpemu {

constexpr int SC_GROUPS_MAX = 16, SC_WAVES = 4, SC_SMAX = GPEMU_MAX_SOURCES;

struct SrcGroup {
  const double *lo, *hi, *mean_part, *vsq_part, *kdiag, *G, *g0, *W, *Q, *w0;
  int64_t Bcap;
  int k, nchunk, nrb, nblk;
};
struct SrcGroups {
  SrcGroup g[SC_GROUPS_MAX];
  int ng, S, ntask, region;           // region: doubles of a wave's matrix area in LDS
  int first[SC_GROUPS_MAX + 1];       // task index of group g's block 0
};

// c_o (lane s < S: its entry) and Z_o (added to Zacc) of observable block o of group gr for proposal b
template <int KP>
__device__ __forceinline__ void source_block_terms(const SrcGroup &gr, int o, int S, int64_t b, int lane, double *M,
                                                   double *Zacc, double &cacc) {
  const int k = gr.k, ldm = k + 1;
  double mu, sd;
  walker_mean_sd<KP>(gr.mean_part, gr.vsq_part, gr.kdiag, nullptr, nullptr, b, gr.Bcap, k, gr.nchunk, gr.nrb, lane, mu, sd);
  const double *Go = gr.G + (int64_t)o * k * k;
  const double *Wo = gr.W + (int64_t)o * k * S;
  double h = lowrank_fill_lds(Go, k, mu, sd, lane, M, ldm);
  h += (lane < k) ? gr.g0[(int64_t)o * k + lane] : 0.0;
  wave_sync_lds();
  (void)wave_cholesky_lds(M, k, ldm, lane);
  // y = L^-1 D^1/2 h and T = L^-1 D^1/2 W_o together, row `lane` in registers
  double y = (lane < k) ? sd * h : 0.0;
  double t[SC_SMAX];
#pragma unroll
  for (int s = 0; s < SC_SMAX; ++s) t[s] = (s < S && lane < k) ? sd * Wo[lane * S + s] : 0.0;
  for (int j = 0; j < k; ++j) {
    const double piv = M[j * ldm + j], lj = (lane > j && lane < k) ? M[lane * ldm + j] : 0.0;
    const double zj = __shfl(y, j) / piv;
    y = (lane == j) ? zj : fma(-lj, zj, y);
#pragma unroll
    for (int s = 0; s < SC_SMAX; ++s) {
      if (s < S) {
        const double zs = __shfl(t[s], j) / piv;
        t[s] = (lane == j) ? zs : fma(-lj, zs, t[s]);
      }
    }
  }
  // c_o = W_o^T m + w0_o - T_o^T y
#pragma unroll
  for (int s = 0; s < SC_SMAX; ++s) {
    if (s < S) {
      const double part = (lane < k) ? fma(Wo[lane * S + s], mu, -t[s] * y) : 0.0;
      const double cs = wave_sum(part) + gr.w0[(int64_t)o * S + s];
      if (lane == s) cacc += cs;
    }
  }
  // Z_o = Q_o - T^T T: T into the (no longer needed) matrix area, then one entry per lane and pass
  wave_sync_lds();
  if (lane < k) {
#pragma unroll
    for (int s = 0; s < SC_SMAX; ++s)
      if (s < S) M[lane * S + s] = t[s];
  }
  wave_sync_lds();
  const double *Qo = gr.Q + (int64_t)o * S * S;
  for (int e = lane; e < S * S; e += 64) {
    const int s1 = e / S, s2 = e - s1 * S;
    double acc = 0.0;
    for (int p = 0; p < k; ++p) acc = fma(M[p * S + s1], M[p * S + s2], acc);
    Zacc[e] += Qo[e] - acc;
  }
  wave_sync_lds();
}

__global__ __launch_bounds__(64 * SC_WAVES) void source_correction_kernel(const double *__restrict__ Xq, SrcGroups sg,
                                                                           double *__restrict__ out, int64_t B, int d,
                                                                           AcceptArgs aa) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x;
  const int S = sg.S;
  const int per_wave = sg.region + S * S;
  double *M = smem + (size_t)wave * per_wave;
  double *Zacc = M + sg.region;
  AcceptOperands ao;
  if (wave == 0) ao = load_accept_operands(Xq, b, lane, aa);
  int64_t ch = 0;                                            // stacked chains: the row's data vector
  if (aa.chain_per && aa.chain_data) ch = (aa.first + b) / aa.chain_per;
  // rows outside any group's box keep their -inf and get no term (every wave decides alike)
  bool inside = true;
  for (int g = 0; g < sg.ng; ++g)
    if (!inside_box(Xq, b, dpad_of(d), d, sg.g[g].lo, sg.g[g].hi, lane)) inside = false;
  for (int e = lane; e < S * S; e += 64) Zacc[e] = 0.0;
  double cacc = 0.0;                                         // lane s < S: entry s of this wave's sum of c_o
  wave_sync_lds();
  if (inside) {
    int g = 0;
    for (int t = wave; t < sg.ntask; t += SC_WAVES) {
      while (t >= sg.first[g + 1]) ++g;
      SrcGroup gr = sg.g[g];
      gr.g0 += ch * gr.nblk * gr.k;
      gr.w0 += ch * gr.nblk * S;
      const int o = t - sg.first[g];
      if (gr.k <= 16) source_block_terms<16>(gr, o, S, b, lane, M, Zacc, cacc);
      else if (gr.k <= 32) source_block_terms<32>(gr, o, S, b, lane, M, Zacc, cacc);
      else source_block_terms<64>(gr, o, S, b, lane, M, Zacc, cacc);
    }
  }
  // this wave's c in LDS behind its Z
  double *cw = smem + (size_t)SC_WAVES * per_wave;
  if (lane < S) cw[wave * SC_SMAX + lane] = cacc;
  __syncthreads();
  if (wave != 0) return;
  double corr = 0.0;
  if (inside) {
    // K = I + sum of the waves' Z (wave order), factored in place in wave 0's accumulator; v = L_K^-1 c
    double *K = Zacc;
    for (int e = lane; e < S * S; e += 64) {
      double z = K[e];
      for (int w = 1; w < SC_WAVES; ++w) z += smem[(size_t)w * per_wave + sg.region + e];
      K[e] = ((e / S == e % S) ? 1.0 : 0.0) + z;
    }
    double c = 0.0;
    if (lane < S) {
      c = cw[lane];
      for (int w = 1; w < SC_WAVES; ++w) c += cw[w * SC_SMAX + lane];
    }
    wave_sync_lds();
    const double logdiag = wave_cholesky_lds(K, S, S, lane);
    const double v = wave_forward_solve_lds(K, S, S, lane, c);
    const double vv = wave_sum((lane < S) ? v * v : 0.0);
    const double ld = wave_sum((lane < S) ? logdiag : 0.0);
    corr = 0.5 * vv - ld;
  }
  // (outside the box: -inf + 0 = -inf)
  finish_walker(corr, out, b, d, lane, 1, aa, ao);
}

int launch_source_correction(gpemu_model *const *ms, int ng, int64_t B, const double *dXq, double *dout, hipStream_t st,
                             const AcceptArgs *aa) {
  if (ng > SC_GROUPS_MAX) {
    set_error("correlated sources: at most %d emulation groups in one evaluation", SC_GROUPS_MAX);
    return GPEMU_ERR_UNSUPPORTED;
  }
  SrcGroups sg;
  memset(&sg, 0, sizeof(sg));
  sg.ng = ng;
  sg.S = ms[0]->n_src;
  int kmax = 1;
  for (int g = 0; g < ng; ++g) {
    const gpemu_model *m = ms[g];
    const Workspace &w = m->ws;
    sg.g[g] = SrcGroup{m->lo, m->hi, w.mean_part, w.vsq_part, m->kdiag, m->G, m->g0, m->W, m->Q, m->w0, w.Bcap,
                       (int)m->k, w.cur_nchunk, w.cur_nrb, (int)m->nblk};
    sg.first[g + 1] = sg.first[g] + (int)m->nblk;
    kmax = std::max(kmax, (int)m->k);
  }
  sg.ntask = sg.first[ng];
  // a wave's area: the k x (k + 1) matrix, later T (k x S)
  sg.region = (int)round_up(std::max(kmax * (kmax + 1), kmax * sg.S), 2);
  const size_t shm = sizeof(double) * ((size_t)SC_WAVES * (sg.region + sg.S * sg.S) + SC_WAVES * SC_SMAX);
  if (shm > 64 * 1024)   // up to k = 64, S = 16: 142 KB
    GP_TRY(allow_dynamic_lds((const void *)source_correction_kernel,
                             (int)(sizeof(double) * (SC_WAVES * (64 * 65 + SC_SMAX * SC_SMAX) + SC_WAVES * SC_SMAX))));
  const AcceptArgs a = aa ? *aa : AcceptArgs();
  hipLaunchKernelGGL(source_correction_kernel, dim3((unsigned)B), dim3(64 * SC_WAVES), shm, st, dXq, sg, dout, B,
                     (int)ms[0]->d, a);
  GP_HIP(hipGetLastError());
  src_path_count(GPEMU_SRC_PATH_CORRECTION);
  if (kmax > 32) src_path_count(GPEMU_SRC_PATH_CORRECTION_K64);
  return GPEMU_OK;
}

}  // namespace gpemu
