// Derivatives with respect to the model parameters x: the Jacobians of the PCs' GP means and variances
// (gpemu_gp_predict_grad) and the gradient of the low-rank log-posterior (gpemu_logpost_grad, gpemu_logpost_groups_grad).
//
//   k_pj(x) = c(r) [+ const],  r^2 = sum_i ((x_i - X_ji) / l_pi)^2,      dk_pj/dx_i = -rho(r) (x_i - X_ji) / l_pi^2
//       RBF / nu = inf: rho = exp(-r^2 / 2);  Matern 1.5: 3 exp(-sqrt3 r);  Matern 2.5: (5/3)(1 + sqrt5 r) exp(-sqrt5 r)
//   m_p = sum_j k_pj alpha_pj,   v_p = max(0, kdiag_p - |W_p k_p|^2),   u_p = W_p^T (W_p k_p)
//   dm_p/dx_i = sum_j alpha_pj dk_pj/dx_i,   dv_p/dx_i = -2 sum_j u_pj dk_pj/dx_i  (0 where the variance was clipped)
//   a_p = dlp/dm_p = -sum_o z_op,  b_p = dlp/dv_p = 1/2 sum_o (z_op^2 - (P_o)_pp),  z_o = U^T Sigma_o^-1 r,
//   P_o = U^T Sigma_o^-1 U, both from the walker's k x k matrix M_o = I + S G_o S = L L^T (S = diag sd):
//       y = L^-1 S h,  t = L^-T y,  z = h - G S t,   Y = L^-1 S G,  (P)_pp = G_pp - |Y_:p|^2
//   dlp/dx_i = sum_p sum_j (a_p alpha_pj - 2 b_p u_pj) dk_pj/dx_i
//
// Per chunk of GRAD_CHUNK = 1024 rows and per group, all on one stream:
//   kmat      K_*^T [k][Npad][Bp] from the raw coordinates (the direct distance, as pcov_kmat_kernel)
//   V         V = W K_*^T, stored (launch_gemm, k_to_m)
//   meanvar   mean = K_* alpha, vsq = sum V^2 in a fixed order; var, and where it was clipped
//   loglik    one wave per (row, observable block), lane = PC: the block's term of lp, a, b; then their sums over
//             the blocks in block order (grad_lik_reduce_kernel)        (the log-posterior only)
//   U         U = W^T V (launch_gemm, k_from_m)
//   contract  partial sums of sum_j g_pj dk_pj/dx_i per (PC, block of GRAD_RB training rows)
//   final     their sum over the row blocks (and the PCs) in index order
// Every element's sums run in an order that depends on the model only: a row's result has the same bits whatever else is
// in the batch and wherever the chunks fall.  No float atomics.
#include <atomic>

#include "internal.h"
#include "gemm.h"
#include "loglik_dev.h"
#include "matern_dev.h"

namespace gpemu {

constexpr int GRAD_CHUNK = 1024;  // rows per pass (bounds the three [k][Npad][chunk] operands: together 3072 / Npad of Wt's size)
constexpr int GRAD_RB = 256;      // training rows per partial sum of the contraction


// ---- K_*^T from the raw coordinates ---------------------------------------------------------------------------------
struct GradKmatArgs {
  const double *Xtr, *X, *ls, *constv;
  double *KT;
  int64_t N, Npad, Bc, Bp, off;
  int d, dp;
};

// blockDim (64, 4): x = column (query row), 4 training rows per thread; grid (Bp / 64, Npad / 16, k).  Zero in the padding.
template <int KIND, int DP>
__global__ __launch_bounds__(256) void grad_kmat_kernel(GradKmatArgs g) {
  const int p = blockIdx.z;
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  double inv[DP], xq[DP];
#pragma unroll
  for (int dd = 0; dd < DP; ++dd) {
    inv[dd] = 1.0 / g.ls[(int64_t)p * g.dp + dd];
    xq[dd] = (dd < g.d && c < g.Bc) ? g.X[(g.off + c) * g.d + dd] : 0.0;
  }
  const double cst = g.constv[p];
  double *o = g.KT + (int64_t)p * g.Npad * g.Bp;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t j = (int64_t)blockIdx.y * 16 + threadIdx.y + 4 * i;
    double v = 0.0;
    if (j < g.N && c < g.Bc) {
      double r2 = 0.0;
#pragma unroll
      for (int dd = 0; dd < DP; ++dd) {
        if (dd < g.d) {
          const double df = (g.Xtr[j * g.dp + dd] - xq[dd]) * inv[dd];
          r2 = fma(df, df, r2);
        }
      }
      v = base_from_r2(KIND, r2) + cst;
    }
    o[j * g.Bp + c] = v;
  }
}

// ---- mean, variance ---------------------------------------------------------------------------------------------------
struct GradMvArgs {
  const double *KT, *V, *alpha, *kdiag;
  double *mean, *var, *clip;     // [Bp][k]; clip: 1 where kdiag - vsq < 0
  int64_t Npad, Bp;
  int k;
};

// blockDim (64, 16), grid (Bp / 64, k): training row j goes to thread row j % 16 -- sixteen chains per element, added
// pairwise in a fixed order ((c_y + c_{y+4}) + (c_{y+8} + c_{y+12}) for y = 0 .. 3, then (s_0 + s_1) + (s_2 + s_3)).
// The padded rows of K_*^T, V and alpha are zero.
__global__ __launch_bounds__(1024) void grad_meanvar_kernel(GradMvArgs g) {
  __shared__ double sm[16][64], sv[16][64];
  const int p = blockIdx.y, tx = threadIdx.x, y = threadIdx.y;
  const int64_t c = (int64_t)blockIdx.x * 64 + tx;
  const double *kt = g.KT + (int64_t)p * g.Npad * g.Bp + c;
  const double *vv = g.V + (int64_t)p * g.Npad * g.Bp + c;
  const double *al = g.alpha + (int64_t)p * g.Npad;
  double ms = 0.0, ss = 0.0;
#pragma unroll 4
  for (int64_t j = y; j < g.Npad; j += 16) {
    const double v = vv[j * g.Bp];
    ms = fma(kt[j * g.Bp], al[j], ms);
    ss = fma(v, v, ss);
  }
  sm[y][tx] = ms;
  sv[y][tx] = ss;
  __syncthreads();
  if (y == 0) {
    double m4[4], s4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      m4[q] = (sm[q][tx] + sm[q + 4][tx]) + (sm[q + 8][tx] + sm[q + 12][tx]);
      s4[q] = (sv[q][tx] + sv[q + 4][tx]) + (sv[q + 8][tx] + sv[q + 12][tx]);
    }
    const double mean = (m4[0] + m4[1]) + (m4[2] + m4[3]);
    const double vsq = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    const double vraw = g.kdiag[p] - vsq;
    g.mean[c * g.k + p] = mean;
    g.var[c * g.k + p] = vraw < 0.0 ? 0.0 : vraw;     // skl _gpr.py:479-485
    g.clip[c * g.k + p] = vraw < 0.0 ? 1.0 : 0.0;
  }
}

// ---- likelihood with adjoints ---------------------------------------------------------------------------------------
struct GradLikArgs {
  const double *X, *lo, *hi, *mean, *var, *clip, *G, *g0, *scal;
  double *tlp, *ta, *tb;         // per (row, block): the block's term of lp [Bc][nblk], of a_p and b_p [Bc][nblk][k]
  double *lp, *wa, *wb;          // lp [B] (at off); wa, wb [Bp][k]: a_p and b_p (b_p = 0 where the variance was clipped)
  int64_t off, Bc;
  int d, k, nblk, accumulate;
};

// One wave per (row, observable block) (one wave per workgroup: k (2 k + 1) doubles of LDS), lane = PC: the blocks'
// factorisations are the serial part, so they run side by side (as loglik_tasks_kernel's do) and grad_lik_reduce_kernel
// adds their terms in block order.  The term is the likelihood's own lowrank_block_term_lds (loglik_dev.h), which also
// fills Y = S G and hands back h and y; the factor L stays in M's lower triangle for the three further solves.  Rows
// outside the box write nothing.
__global__ __launch_bounds__(64) void grad_loglik_kernel(GradLikArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x, k = g.k, ldm = k + 1;
  const int64_t c = blockIdx.x, b = g.off + c;
  const int o = blockIdx.y;
  double *M = smem, *Y = smem + (size_t)k * ldm;
  if (!inside_box(g.X, b, g.d, g.d, g.lo, g.hi, lane)) return;
  double mu = 0.0, sd = 0.0;
  if (lane < k) {
    mu = g.mean[c * k + lane];
    sd = sqrt(g.var[c * k + lane]);
  }
  double av = 0.0, bv = 0.0;
  const double *Go = g.G + (int64_t)o * k * k;
  double h, y;   // h = G_o m + g0_o, y = L^-1 (S h)
  const double total =
      lowrank_block_term_lds<true>(Go, g.g0 + (int64_t)o * k, g.scal + 2 * o, k, mu, sd, lane, M, ldm, h, y, Y);
  // Y_:lane = L^-1 (S G)_:lane, lane = right-hand side: L's entries are broadcast reads, Y's are conflict free
  double ynorm = 0.0;
  if (lane < k) {
    for (int i = 0; i < k; ++i) {
      double s = Y[i * k + lane];
      for (int j = 0; j < i; ++j) s = fma(-M[i * ldm + j], Y[j * k + lane], s);
      s /= M[i * ldm + i];
      Y[i * k + lane] = s;
      ynorm = fma(s, s, ynorm);
    }
  }
  // t = L^-T y, rows from the last up: row j of L is read along the lanes
  double tt = y;
  for (int j = k - 1; j >= 0; --j) {
    const double tj = __shfl(tt, j) / M[j * ldm + j];
    if (lane == j) tt = tj;
    if (lane < j) tt = fma(-M[j * ldm + lane], tj, tt);
  }
  // z = h - G S t
  const double st = sd * tt;
  double z = h;
  for (int q = 0; q < k; ++q) {
    const double gq = (lane < k) ? Go[q * k + lane] : 0.0;
    z = fma(-gq, __shfl(st, q), z);
  }
  if (lane < k) {
    const double pdiag = Go[lane * k + lane] - ynorm;
    av -= z;
    bv += 0.5 * (z * z - pdiag);
  }
  const int64_t term = c * g.nblk + o;
  if (lane < k) {
    g.ta[term * k + lane] = av;
    g.tb[term * k + lane] = bv;
  }
  if (lane == 0) g.tlp[term] = total;
}

// the blocks' terms added in block order, per (row, PC): a_p, b_p (0 where the variance was clipped), and the row's lp
// (-inf and zero weights outside the open box; + the groups before this one)
__global__ __launch_bounds__(256) void grad_lik_reduce_kernel(GradLikArgs g) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = idx / g.k;
  const int p = (int)(idx - c * g.k);
  if (c >= g.Bc) return;
  const int64_t b = g.off + c;
  bool inside = true;
  for (int i = 0; i < g.d; ++i) {
    const double x = g.X[b * g.d + i];
    inside = inside && (x > g.lo[i]) && (x < g.hi[i]);
  }
  double av = 0.0, bv = 0.0, total = -INFINITY;
  if (inside) {
    total = 0.0;
    for (int o = 0; o < g.nblk; ++o) {
      const int64_t t = c * g.nblk + o;
      av += g.ta[t * g.k + p];
      bv += g.tb[t * g.k + p];
      total += g.tlp[t];
    }
  }
  g.wa[c * g.k + p] = av;
  g.wb[c * g.k + p] = (inside && g.clip[c * g.k + p] == 0.0) ? bv : 0.0;
  if (p == 0) g.lp[b] = g.accumulate ? total + g.lp[b] : total;
}

// ---- the kernel-derivative contraction ------------------------------------------------------------------------------
struct GradConArgs {
  const double *Xtr, *X, *ls, *alpha, *U, *wa, *wb, *clip;
  double *partA, *partB;         // [k][nrb][Bp][DP]  (partB: the variance's, Jacobian form only)
  int64_t N, Npad, Bc, Bp, off;
  int d, dp, k, nrb;
};

template <int KIND>
__device__ __forceinline__ double grad_rho(double r2) {
  if (KIND == 0) return exp(-0.5 * r2);
  const double r = sqrt(r2);
  if (KIND == 2) return 3.0 * exp(-1.7320508075688772 * r);
  const double t = 2.23606797749979 * r;
  return (5.0 / 3.0) * (1.0 + t) * exp(-t);
}

// blockDim (64, 4): x = query row, a wave per y; grid (Bp / 64, nrb, k).  Training row j of row block rb goes to wave
// (j - rb GRAD_RB) % 4; the four waves' sums are added through LDS in wave order.  The training row is the same for the
// whole wave (scalar loads); the query and 1 / l stay in registers.  JAC: the two Jacobians' sums, weights (1, 0) and
// (0, 1), instead of the one weighted by (a_p, b_p).
template <int KIND, int DP, bool JAC>
__global__ __launch_bounds__(256) void grad_contract_kernel(GradConArgs g) {
  __shared__ double red[4][DP][64];
  const int p = blockIdx.z, rb = blockIdx.y, tx = threadIdx.x;
  const int y = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int64_t c = (int64_t)blockIdx.x * 64 + tx;
  const bool active = c < g.Bc;
  double inv[DP], xq[DP], accA[DP], accB[JAC ? DP : 1];
#pragma unroll
  for (int dd = 0; dd < DP; ++dd) {
    inv[dd] = 1.0 / g.ls[(int64_t)p * g.dp + dd];
    xq[dd] = (dd < g.d && active) ? g.X[(g.off + c) * g.d + dd] : 0.0;
    accA[dd] = 0.0;
    if (JAC) accB[dd] = 0.0;
  }
  double wa = 0.0, wb = 0.0;
  if (active) {
    wa = JAC ? 1.0 : g.wa[c * g.k + p];
    wb = JAC ? (g.clip[c * g.k + p] != 0.0 ? 0.0 : 1.0) : g.wb[c * g.k + p];
  }
  const bool work = active && (JAC || wa != 0.0 || wb != 0.0);      // rows outside the box carry (0, 0)
  const double *al = g.alpha + (int64_t)p * g.Npad;
  const double *up = g.U + (int64_t)p * g.Npad * g.Bp + c;
  const int64_t j1 = ((int64_t)(rb + 1) * GRAD_RB < g.N) ? (int64_t)(rb + 1) * GRAD_RB : g.N;
  if (work) {
    for (int64_t j = (int64_t)rb * GRAD_RB + y; j < j1; j += 4) {
      const double *xj = g.Xtr + j * g.dp;
      double df[DP];
      double r2 = 0.0;
#pragma unroll
      for (int dd = 0; dd < DP; ++dd) {
        df[dd] = (dd < g.d) ? (xq[dd] - xj[dd]) * inv[dd] : 0.0;
        r2 = fma(df[dd], df[dd], r2);
      }
      const double rho = grad_rho<KIND>(r2);
      const double uj = up[j * g.Bp], aj = al[j];
      if (JAC) {
        const double ga = -rho * aj, gb = 2.0 * rho * uj * wb;
#pragma unroll
        for (int dd = 0; dd < DP; ++dd) {
          const double e = df[dd] * inv[dd];
          accA[dd] = fma(ga, e, accA[dd]);
          accB[dd] = fma(gb, e, accB[dd]);
        }
      } else {
        const double gg = -rho * fma(wa, aj, -2.0 * wb * uj);
#pragma unroll
        for (int dd = 0; dd < DP; ++dd) accA[dd] = fma(gg, df[dd] * inv[dd], accA[dd]);
      }
    }
  }
#pragma unroll
  for (int dd = 0; dd < DP; ++dd) red[y][dd][tx] = accA[dd];
  __syncthreads();
  if (y == 0 && active) {
    double *o = g.partA + (((int64_t)p * g.nrb + rb) * g.Bp + c) * DP;
#pragma unroll
    for (int dd = 0; dd < DP; ++dd) o[dd] = (red[0][dd][tx] + red[1][dd][tx]) + (red[2][dd][tx] + red[3][dd][tx]);
  }
  if (JAC) {
    __syncthreads();
#pragma unroll
    for (int dd = 0; dd < DP; ++dd) red[y][dd][tx] = accB[dd];
    __syncthreads();
    if (y == 0 && active) {
      double *o = g.partB + (((int64_t)p * g.nrb + rb) * g.Bp + c) * DP;
#pragma unroll
      for (int dd = 0; dd < DP; ++dd) o[dd] = (red[0][dd][tx] + red[1][dd][tx]) + (red[2][dd][tx] + red[3][dd][tx]);
    }
  }
}

// grad[off + c][i] = sum_p sum_rb part[p][rb][c][i] in index order (+ the groups before this one); 0 where lp = -inf,
// NaN where lp is NaN
__global__ __launch_bounds__(256) void grad_final_kernel(const double *__restrict__ part, const double *__restrict__ lp,
                                                         double *__restrict__ grad, int64_t Bc, int64_t Bp, int64_t off,
                                                         int d, int DP, int k, int nrb, int accumulate) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = idx / DP;
  const int i = (int)(idx - c * DP);
  if (c >= Bc || i >= d) return;
  double s = 0.0;
  for (int q = 0; q < k * nrb; ++q) s += part[((int64_t)q * Bp + c) * DP + i];
  double *o = grad + (off + c) * d + i;
  if (accumulate) s = *o + s;
  const double l = lp[off + c];
  if (l == -INFINITY) s = 0.0;        // outside the box
  else if (l != l) s = l;             // a NaN log-posterior (a covariance that is not positive definite): NaN, not a 0 that looks valid
  *o = s;
}

// the Jacobians [B][k][d] from the two sets of partial sums; mean, var [B][k] from the chunk's
__global__ __launch_bounds__(256) void grad_final_jac_kernel(const double *__restrict__ partA, const double *__restrict__ partB,
                                                             const double *__restrict__ cmean, const double *__restrict__ cvar,
                                                             double *__restrict__ mean, double *__restrict__ var,
                                                             double *__restrict__ dmean, double *__restrict__ dvar, int64_t Bc,
                                                             int64_t Bp, int64_t off, int d, int DP, int k, int nrb) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(idx % DP);
  const int64_t cp = idx / DP;
  const int p = (int)(cp % k);
  const int64_t c = cp / k;
  if (c >= Bc) return;
  if (i == 0) {
    if (mean) mean[(off + c) * k + p] = cmean[c * k + p];
    if (var) var[(off + c) * k + p] = cvar[c * k + p];
  }
  if (i >= d) return;
  double sa = 0.0, sb = 0.0;
  for (int rb = 0; rb < nrb; ++rb) {
    const int64_t at = (((int64_t)p * nrb + rb) * Bp + c) * DP + i;
    sa += partA[at];
    sb += partB[at];
  }
  dmean[((off + c) * k + p) * d + i] = sa;
  dvar[((off + c) * k + p) * d + i] = sb;
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct GradWs {
  double *KT, *V, *U, *mean, *var, *clip, *wa, *wb, *partA, *partB;
  double *tlp, *ta, *tb;         // the likelihood's per-block terms (grad_lik_workspace)
  int nrb;
};

static int64_t grad_ws_doubles(const gpemu_model *m) {
  const int64_t nrb = (m->N + GRAD_RB - 1) / GRAD_RB;
  return 3 * m->k * m->Npad * GRAD_CHUNK + 5 * GRAD_CHUNK * m->k + 2 * m->k * nrb * GRAD_CHUNK * m->dp;
}

// the workspace of the gradient calls, allocated by the first of them (a model that never asks allocates nothing)
static int grad_workspace(gpemu_model *m, GradWs &w) {
  if (!m->grad_ws) GP_TRY(dev_alloc(&m->grad_ws, grad_ws_doubles(m)));
  const int64_t big = m->k * m->Npad * GRAD_CHUNK, sm = GRAD_CHUNK * m->k;
  w.nrb = (int)((m->N + GRAD_RB - 1) / GRAD_RB);
  double *q = m->grad_ws;
  w.KT = q; q += big;
  w.V = q; q += big;
  w.U = q; q += big;
  w.mean = q; q += sm;
  w.var = q; q += sm;
  w.clip = q; q += sm;
  w.wa = q; q += sm;
  w.wb = q; q += sm;
  w.partA = q; q += m->k * w.nrb * GRAD_CHUNK * m->dp;
  w.partB = q;
  return GPEMU_OK;
}

// the per-(row, block) terms of the likelihood: sized by the number of observable blocks, which a new likelihood setup
// may change
static int grad_lik_workspace(gpemu_model *m, GradWs &w, hipStream_t st) {
  const int64_t need = (int64_t)GRAD_CHUNK * m->nblk * (2 * m->k + 1);
  GP_TRY(dev_reserve(&m->grad_lik_cap, need, {st}, {dev_field(&m->grad_lik_ws, need)}));
  w.tlp = m->grad_lik_ws;
  w.ta = w.tlp + (int64_t)GRAD_CHUNK * m->nblk;
  w.tb = w.ta + (int64_t)GRAD_CHUNK * m->nblk * m->k;
  return GPEMU_OK;
}

// what the derivative kernels cover: the kernels whose derivative is finite and continuous at r = 0
static int grad_supported(const gpemu_model *m, const char *what) {
  const int kind = kstar_kind(m);
  if (kind == 1 || kind == 4) {
    set_error("%s: the Matern kernel of nu = %g is not supported (its derivative needs K_{nu-1} and is singular or "
              "discontinuous at r = 0 for nu < 1): nu = 1.5, 2.5 or inf (RBF) only", what, m->nu);
    return GPEMU_ERR_UNSUPPORTED;
  }
  return GPEMU_OK;
}

int grad_lik_supported(const gpemu_model *m, const char *what) {
  GP_TRY(grad_supported(m, what));
  if (!m->lik_ready) { set_error("gpemu_likelihood_setup has not been called"); return GPEMU_ERR_STATE; }
  if (m->n_src > 0) {
    set_error("%s: groups with correlated systematic sources (n_src = %d) are not supported", what, m->n_src);
    return GPEMU_ERR_UNSUPPORTED;
  }
  if (m->lik_chains != 1) {
    set_error("%s: a likelihood set up for %d data vectors is not supported (one only)", what, m->lik_chains);
    return GPEMU_ERR_UNSUPPORTED;
  }
  return GPEMU_OK;
}

// K_*^T, V, mean / var and U of the chunk [off, off + Bc) of dX; lik: the likelihood launch between V and U
static int grad_chunk_front(gpemu_model *m, const GradWs &w, int64_t off, int64_t Bc, const double *dX, double *dlp,
                            int accumulate, bool lik, hipStream_t st) {
  const int64_t Bp = round_up(Bc, 64), Np = m->Npad;
  const int k = (int)m->k;
  GradKmatArgs ka{m->Xtr, dX, m->ls, m->constv, w.KT, m->N, Np, Bc, Bp, off, (int)m->d, m->dp};
  const dim3 kgrid((unsigned)(Bp / 64), (unsigned)(Np / 16), (unsigned)k), blk(64, 4);
  GP_TRY(with_base_kind(kstar_kind(m), [&](auto kd) {
    constexpr int K = decltype(kd)::value;
    if constexpr (K == 0 || K == 2 || K == 3) {       // (grad_supported has declined the others: no instance of them)
      if (m->dp == DPAD) hipLaunchKernelGGL((grad_kmat_kernel<K, DPAD>), kgrid, blk, 0, st, ka);
      else hipLaunchKernelGGL((grad_kmat_kernel<K, DPAD_WIDE>), kgrid, blk, 0, st, ka);
      return GPEMU_OK;
    } else {
      set_error("gradient: unsupported base kernel %d", K);
      return GPEMU_ERR_UNSUPPORTED;
    }
  }));
  GP_HIP(hipGetLastError());
  GemmArgs gv;   // V = W K_*^T: W = Wt^T lower triangular
  gv.A = m->Wt; gv.lda = Np; gv.strideA = Np * Np;
  gv.B = w.KT; gv.ldb = Bp; gv.strideB = Np * Bp;
  gv.C = w.V; gv.ldc = Bp; gv.strideC = Np * Bp;
  gv.M = (int)Np; gv.N = (int)Bp; gv.K = (int)Np;
  gv.k_to_m = 1;
  GP_TRY(launch_gemm(gv, true, true, k, st));
  GradMvArgs mv{w.KT, w.V, m->alpha, m->kdiag, w.mean, w.var, w.clip, Np, Bp, k};
  hipLaunchKernelGGL(grad_meanvar_kernel, dim3((unsigned)(Bp / 64), (unsigned)k), dim3(64, 16), 0, st, mv);
  GP_HIP(hipGetLastError());
  if (lik) {
    GradLikArgs la{dX, m->lo, m->hi, w.mean, w.var, w.clip, m->G, m->g0, m->scal, w.tlp, w.ta, w.tb, dlp, w.wa, w.wb, off, Bc,
                   (int)m->d, k, (int)m->nblk, accumulate};
    const size_t shm = sizeof(double) * (size_t)k * (2 * k + 1);
    if (shm > 64 * 1024) GP_TRY(allow_dynamic_lds((const void *)grad_loglik_kernel, (int)(sizeof(double) * 64 * 129)));
    hipLaunchKernelGGL(grad_loglik_kernel, dim3((unsigned)Bc, (unsigned)m->nblk), dim3(64), shm, st, la);
    hipLaunchKernelGGL(grad_lik_reduce_kernel, dim3((unsigned)((Bc * k + 255) / 256)), dim3(256), 0, st, la);
    GP_HIP(hipGetLastError());
    grad_path_count(GPEMU_GRAD_PATH_LOGLIK);
  }
  GemmArgs gu;   // U = W^T V: Wt [m][k] upper triangular
  gu.A = m->Wt; gu.lda = Np; gu.strideA = Np * Np;
  gu.B = w.V; gu.ldb = Bp; gu.strideB = Np * Bp;
  gu.C = w.U; gu.ldc = Bp; gu.strideC = Np * Bp;
  gu.M = (int)Np; gu.N = (int)Bp; gu.K = (int)Np;
  gu.k_from_m = 1;
  GP_TRY(launch_gemm(gu, false, true, k, st));
  grad_path_count(GPEMU_GRAD_PATH_CHUNK);
  return GPEMU_OK;
}

template <bool JAC>
static int grad_chunk_contract(gpemu_model *m, const GradWs &w, int64_t off, int64_t Bc, const double *dX, hipStream_t st) {
  const int64_t Bp = round_up(Bc, 64);
  GradConArgs ca{m->Xtr, dX, m->ls, m->alpha, w.U, w.wa, w.wb, w.clip, w.partA, w.partB, m->N, m->Npad, Bc, Bp, off,
                 (int)m->d, m->dp, (int)m->k, w.nrb};
  const dim3 grid((unsigned)(Bp / 64), (unsigned)w.nrb, (unsigned)m->k), blk(64, 4);
  GP_TRY(with_base_kind(kstar_kind(m), [&](auto kd) {
    constexpr int K = decltype(kd)::value;
    if constexpr (K == 0 || K == 2 || K == 3) {
      if (m->dp == DPAD) hipLaunchKernelGGL((grad_contract_kernel<K, DPAD, JAC>), grid, blk, 0, st, ca);
      else hipLaunchKernelGGL((grad_contract_kernel<K, DPAD_WIDE, JAC>), grid, blk, 0, st, ca);
      return GPEMU_OK;
    } else {
      set_error("gradient: unsupported base kernel %d", K);
      return GPEMU_ERR_UNSUPPORTED;
    }
  }));
  GP_HIP(hipGetLastError());
  grad_path_count(m->dp == DPAD ? (JAC ? GPEMU_GRAD_PATH_JACOBIAN_8 : GPEMU_GRAD_PATH_CONTRACT_8)
                                : (JAC ? GPEMU_GRAD_PATH_JACOBIAN_16 : GPEMU_GRAD_PATH_CONTRACT_16));
  return GPEMU_OK;
}

// lp [B] and grad [B][d] of dX [B][d] summed over ng groups (all checked by the caller); asynchronous on st
int logpost_grad_eval(gpemu_model *const *ms, int ng, int64_t B, const double *dX, double *dlp, double *dgrad,
                             hipStream_t st) {
  for (int64_t off = 0; off < B; off += GRAD_CHUNK) {
    const int64_t Bc = (B - off < GRAD_CHUNK) ? (B - off) : GRAD_CHUNK, Bp = round_up(Bc, 64);
    for (int g = 0; g < ng; ++g) {
      gpemu_model *m = ms[g];
      GradWs w;
      GP_TRY(grad_workspace(m, w));
      GP_TRY(grad_lik_workspace(m, w, st));
      GP_TRY(grad_chunk_front(m, w, off, Bc, dX, dlp, g > 0, true, st));
      GP_TRY(grad_chunk_contract<false>(m, w, off, Bc, dX, st));
      hipLaunchKernelGGL(grad_final_kernel, dim3((unsigned)((Bc * m->dp + 255) / 256)), dim3(256), 0, st, w.partA, dlp,
                         dgrad, Bc, Bp, off, (int)m->d, m->dp, (int)m->k, w.nrb, g > 0 ? 1 : 0);
      GP_HIP(hipGetLastError());
    }
  }
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_gp_predict_grad_dev(gpemu_model *m, int64_t B, const double *dX, double *dmean, double *dvar, double *ddmean,
                              double *ddvar, void *stream) {
  GP_ARG(m, "null pointer");
  GP_ARG(B >= 0, "B must not be negative");
  GP_TRY(grad_supported(m, "gp_predict_grad"));
  if (B == 0) return GPEMU_OK;
  GP_ARG(dX && ddmean && ddvar, "null pointer");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  GradWs w;
  w.tlp = w.ta = w.tb = nullptr;
  GP_TRY(grad_workspace(m, w));
  for (int64_t off = 0; off < B; off += GRAD_CHUNK) {
    const int64_t Bc = (B - off < GRAD_CHUNK) ? (B - off) : GRAD_CHUNK, Bp = round_up(Bc, 64);
    GP_TRY(grad_chunk_front(m, w, off, Bc, dX, nullptr, 0, false, st));
    GP_TRY(grad_chunk_contract<true>(m, w, off, Bc, dX, st));
    hipLaunchKernelGGL(grad_final_jac_kernel, dim3((unsigned)((Bc * m->k * m->dp + 255) / 256)), dim3(256), 0, st, w.partA,
                       w.partB, w.mean, w.var, dmean, dvar, ddmean, ddvar, Bc, Bp, off, (int)m->d, m->dp, (int)m->k, w.nrb);
    GP_HIP(hipGetLastError());
  }
  return GPEMU_OK;
}

int gpemu_gp_predict_grad(gpemu_model *m, int64_t B, const double *X, double *mean, double *var, double *dmean_dx,
                          double *dvar_dx) {
  GP_ARG(m, "null pointer");
  GP_ARG(B >= 0, "B must not be negative");
  GP_TRY(grad_supported(m, "gp_predict_grad"));
  if (B == 0) return GPEMU_OK;
  GP_ARG(X && mean && var && dmean_dx && dvar_dx, "null pointer");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int64_t d = m->d, k = m->k;
  DevScope sc(st);
  double *dX, *dm, *dv, *ddm, *ddv;
  GP_TRY(sc.alloc(&dX, B * d));
  GP_TRY(sc.alloc(&dm, B * k));
  GP_TRY(sc.alloc(&dv, B * k));
  GP_TRY(sc.alloc(&ddm, B * k * d));
  GP_TRY(sc.alloc(&ddv, B * k * d));
  GP_TRY(upload(dX, X, B * d, st));
  GP_TRY(gpemu_gp_predict_grad_dev(m, B, dX, dm, dv, ddm, ddv, st));
  GP_TRY(sc.download(mean, dm, B * k));
  GP_TRY(sc.download(var, dv, B * k));
  GP_TRY(sc.download(dmean_dx, ddm, B * k * d));
  GP_TRY(sc.download(dvar_dx, ddv, B * k * d));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_logpost_grad_dev(gpemu_model *m, int64_t B, const double *dX, double *dlp, double *dgrad, int mode, void *stream) {
  GP_ARG(m, "null pointer");
  GP_ARG(B >= 0, "B must not be negative");
  GP_ARG(mode == GPEMU_LOGPOST_LOWRANK || mode == GPEMU_LOGPOST_EXACT, "mode");
  if (mode == GPEMU_LOGPOST_EXACT) {
    set_error("logpost_grad: GPEMU_LOGPOST_EXACT has no gradient: use GPEMU_LOGPOST_LOWRANK");
    return GPEMU_ERR_UNSUPPORTED;
  }
  GP_TRY(grad_lik_supported(m, "logpost_grad"));
  if (B == 0) return GPEMU_OK;
  GP_ARG(dX && dlp && dgrad, "null pointer");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  return logpost_grad_eval(&m, 1, B, dX, dlp, dgrad, st);
}

int gpemu_logpost_groups_grad(gpemu_model *const *models, int n_groups, int64_t B, const double *X, double *lp,
                              double *grad, int mode) {
  GP_ARG(models && n_groups > 0, "models");
  GP_ARG(B >= 0, "B must not be negative");
  GP_ARG(mode == GPEMU_LOGPOST_LOWRANK || mode == GPEMU_LOGPOST_EXACT, "mode");
  for (int g = 0; g < n_groups; ++g) {
    GP_ARG(models[g], "null model");
    GP_ARG(models[g]->d == models[0]->d && models[g]->device == models[0]->device,
           "models must share the parameter dimension and the device");
  }
  if (mode == GPEMU_LOGPOST_EXACT) {
    set_error("logpost_grad: GPEMU_LOGPOST_EXACT has no gradient: use GPEMU_LOGPOST_LOWRANK");
    return GPEMU_ERR_UNSUPPORTED;
  }
  for (int g = 0; g < n_groups; ++g) GP_TRY(grad_lik_supported(models[g], "logpost_grad"));
  if (B == 0) return GPEMU_OK;
  GP_ARG(X && lp && grad, "null pointer");
  gpemu_model *m0 = models[0];
  GP_HIP(hipSetDevice(m0->device));
  hipStream_t st = m0->stream;
  const int64_t d = m0->d;
  // the other groups' streams may still hold work on their models (a likelihood setup): the evaluation runs on the first's
  for (int g = 1; g < n_groups; ++g) GP_HIP(hipStreamSynchronize(models[g]->stream));
  DevScope sc(st);
  double *dX, *dlp, *dgrad;
  GP_TRY(sc.alloc(&dX, B * d));
  GP_TRY(sc.alloc(&dlp, B));
  GP_TRY(sc.alloc(&dgrad, B * d));
  GP_TRY(upload(dX, X, B * d, st));
  GP_TRY(logpost_grad_eval(models, n_groups, B, dX, dlp, dgrad, st));
  GP_TRY(sc.download(lp, dlp, B));
  GP_TRY(sc.download(grad, dgrad, B * d));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_logpost_grad(gpemu_model *m, int64_t B, const double *X, double *lp, double *grad, int mode) {
  GP_ARG(m, "null pointer");
  return gpemu_logpost_groups_grad(&m, 1, B, X, lp, grad, mode);
}

}  // extern "C"
