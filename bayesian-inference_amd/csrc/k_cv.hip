// Cross-validation of a fitted emulation group at its fitted theta (gpemu_model_cross_validate).
//
// With A = K^-1 = Wt Wt^T (Wt = (L^-1)^T, resident for every PC) and a fold I of m held-out points (R&W 5.4.2, the block
// form of the leave-one-out identities):
//   mu_I    = y_I - (A_II)^-1 alpha_I
//   Sigma_I = (A_II)^-1                       (covariance of y_I given the other folds, alpha jitter on its diagonal)
//   var_i   = Sigma_ii - jitter, clipped at 0 (skl _gpr.py:479-485 on the fit of the other folds)
// Per (PC, fold) problem:
//   gather   G = Wt[I, r0 ..]  (r0 = min I: Wt[a][r] = 0 for r < a), rows padded with zeros to mp = 64 ceil(m / 64)
//   SYRK     A_II = G G^T (lower tiles; launch_gemm, one batched launch per fold), padded diagonal set to 1
//   factor   A_II = C C^T and M = C^-1 (device_cholesky_blocked + device_trtri_blocked, batched over the chunk)
//   epilogue u = M alpha_I (one wave per row), then per column l: v_l = (M^T u)_l, s_l = ||M e_l||^2
//            mean = y - v, var = max(s - jitter, 0)
// Leave-one-out (every fold one point) needs no factorisation: A_ii = ||Wt[p] row i||^2 (cv_loo_kernel).
// Every sum runs in a fixed order (lane-strided partial sums, then a fixed butterfly): the results are reproducible bit
// for bit, and independent of how the problems are dealt into chunks.
#include "internal.h"
#include "gemm.h"
#include "wave_dev.h"

namespace gpemu {

constexpr int CV_NB = 64;   // padding unit of the fold operands (launch_gemm, the blocked Cholesky)

// LOO: one wave per (point i, PC p).  Row i of Wt[p] is non-zero in columns [i, N) only.
__global__ __launch_bounds__(256) void cv_loo_kernel(const double *__restrict__ Wt, int64_t Npad, int N, int k,
                                                     const double *__restrict__ alpha, const double *__restrict__ jit,
                                                     const double *__restrict__ y, double *__restrict__ mean,
                                                     double *__restrict__ var) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int p = blockIdx.y;
  if (i >= N) return;
  const double *row = Wt + (int64_t)p * Npad * Npad + (int64_t)i * Npad;
  double s = 0.0;
  for (int r = i + lane; r < N; r += 64) s = fma(row[r], row[r], s);
  s = wave_sum(s);
  if (lane == 0) {
    const double sig = 1.0 / s;
    mean[(int64_t)i * k + p] = y[(int64_t)i * k + p] - alpha[(int64_t)p * Npad + i] * sig;
    const double v = sig - jit[p];
    var[(int64_t)i * k + p] = v < 0.0 ? 0.0 : v;
  }
}

// Problems of a chunk: q = q0 + z, fold f = q / k, PC p = q % k (fold-major).  idx[foff[f] ..] = the fold's points in
// ascending order.
struct CvChunk {
  const double *Wt = nullptr;
  const double *alpha = nullptr;
  const double *jit = nullptr;
  const double *y = nullptr;
  const int *idx = nullptr;
  const int *foff = nullptr;
  double *G = nullptr;       // [nprob][mp][Kcap]
  double *A = nullptr;       // [nprob][mp][mp]  A_II, then its factor C
  double *W = nullptr;       // [nprob][mp][mp]  M = C^-1
  double *u = nullptr;       // [nprob][mp]
  double *mean = nullptr;    // [N][k]
  double *var = nullptr;     // [N][k]
  int64_t Npad = 0, Kcap = 0, mp = 0;
  int N = 0, k = 0, q0 = 0;
};

// row q of G for problem z: G[z][q][c] = Wt[p][I_q][r0 + c] (zero for q >= m or r0 + c >= N)
__global__ __launch_bounds__(256) void cv_gather_kernel(CvChunk c) {
  const int q = blockIdx.x, z = blockIdx.y;
  const int qq = c.q0 + z, f = qq / c.k, p = qq % c.k;
  const int start = c.foff[f], m = c.foff[f + 1] - start;
  const int r0 = c.idx[start];
  double *g = c.G + ((int64_t)z * c.mp + q) * c.Kcap;
  const double *row = q < m ? c.Wt + (int64_t)p * c.Npad * c.Npad + (int64_t)c.idx[start + q] * c.Npad + r0 : nullptr;
  for (int64_t col = threadIdx.x; col < c.Kcap; col += 256) g[col] = (row && r0 + col < c.N) ? row[col] : 0.0;
}

// the padded diagonal of A_II: identity, so that the padded problem stays positive definite and falls out of the solve
__global__ void cv_pad_diag_kernel(CvChunk c) {
  const int z = blockIdx.x;
  const int qq = c.q0 + z, f = qq / c.k;
  const int m = c.foff[f + 1] - c.foff[f];
  for (int q = m + (int)threadIdx.x; q < c.mp; q += blockDim.x) c.A[(int64_t)z * c.mp * c.mp + (int64_t)q * c.mp + q] = 1.0;
}

// u = M alpha_I: one wave per row j < m (M lower triangular)
__global__ __launch_bounds__(256) void cv_u_kernel(CvChunk c) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), z = blockIdx.y;
  const int qq = c.q0 + z, f = qq / c.k, p = qq % c.k;
  const int start = c.foff[f], m = c.foff[f + 1] - start;
  if (j >= m) return;
  const double *row = c.W + (int64_t)z * c.mp * c.mp + (int64_t)j * c.mp;
  const double *al = c.alpha + (int64_t)p * c.Npad;
  double s = 0.0;
  for (int l = lane; l <= j; l += 64) s = fma(row[l], al[c.idx[start + l]], s);
  s = wave_sum(s);
  if (lane == 0) c.u[(int64_t)z * c.mp + j] = s;
}

// per held-out point l: v = (M^T u)_l, s = sum_j M[j][l]^2 (column l of M, rows j >= l); one thread per column
__global__ __launch_bounds__(256) void cv_out_kernel(CvChunk c) {
  const int l = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
  const int qq = c.q0 + z, f = qq / c.k, p = qq % c.k;
  const int start = c.foff[f], m = c.foff[f + 1] - start;
  if (l >= m) return;
  const double *Wz = c.W + (int64_t)z * c.mp * c.mp;
  const double *u = c.u + (int64_t)z * c.mp;
  double v = 0.0, s = 0.0;
  for (int j = l; j < m; ++j) {
    const double w = Wz[(int64_t)j * c.mp + l];
    v = fma(w, u[j], v);
    s = fma(w, w, s);
  }
  const int64_t i = c.idx[start + l];
  c.mean[i * c.k + p] = c.y[i * c.k + p] - v;
  const double vr = s - c.jit[p];
  c.var[i * c.k + p] = vr < 0.0 ? 0.0 : vr;
}

// observable space (ref: emulation.py:516-548 for one sample, n_div = 1), one thread per (point, feature):
//   central_value = (sum_p mean_p comp[p][f]) scale_f + mean_f
//   variance      = (sum_p comp[p][f] var_p comp[p][f] + cov_unexplained[f][f]) scale_f^2
__global__ __launch_bounds__(256) void cv_backproject_kernel(const double *__restrict__ mean, const double *__restrict__ var,
                                                             const double *__restrict__ comp, const double *__restrict__ smean,
                                                             const double *__restrict__ sscale,
                                                             const double *__restrict__ cunexpl, int k, int F,
                                                             double *__restrict__ cv, double *__restrict__ vo) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  const int64_t i = blockIdx.y;
  if (f >= F) return;
  double a = 0.0, b = 0.0;
  for (int p = 0; p < k; ++p) {
    const double s = comp[(int64_t)p * F + f];
    a = fma(mean[i * k + p], s, a);
    b = fma(s * var[i * k + p], s, b);
  }
  const double sc = sscale[f];
  if (cv) cv[i * F + f] = a * sc + smean[f];
  if (vo) vo[i * F + f] = (b + cunexpl[(int64_t)f * F + f]) * (sc * sc);
}

// Everything on m->stream.  idx / foff / y / mean / var are device arrays (see gpemu_model_cross_validate);
// max_chunk > 0 caps the problems per chunk (tests).  hfoff: the fold offsets on the host, hr0: first point per fold.
int cross_validate(gpemu_model *m, int n_folds, const int *didx, const int *dfoff, const std::vector<int> &hfoff,
                   const std::vector<int> &hr0, const double *dy, double *dmean, double *dvar, int64_t max_chunk) {
  hipStream_t st = m->stream;
  const int N = (int)m->N, k = (int)m->k;
  int mmax = 0;
  for (int f = 0; f < n_folds; ++f) mmax = std::max(mmax, hfoff[f + 1] - hfoff[f]);
  if (mmax == 1) {
    hipLaunchKernelGGL(cv_loo_kernel, dim3((unsigned)((N + 3) / 4), (unsigned)k), dim3(256), 0, st, m->Wt, m->Npad, N, k,
                       m->alpha, m->cv_jit, dy, dmean, dvar);
    GP_HIP(hipGetLastError());
    return GPEMU_OK;
  }
  const int64_t mp = round_up(mmax, CV_NB), Kcap = round_up(N, 16);
  const int64_t nprob = (int64_t)n_folds * k;
  // problems per chunk: a quarter of the free device memory (at most 8 GiB), at most 16384 * 64 / mp (grid limits of the
  // batched Cholesky / inverse), and the caller's cap
  const int64_t per = mp * Kcap + 3 * mp * mp + mp * CV_NB + mp;     // doubles: G, A, W, T, Dinv, u
  size_t fb = 0, tb = 0;
  GP_HIP(hipMemGetInfo(&fb, &tb));
  const int64_t budget = std::min<int64_t>((int64_t)(fb / 4), (int64_t)8 << 30);
  int64_t chunk = std::max<int64_t>(1, budget / (8 * per));
  chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, 16384 * 64 / mp));
  if (max_chunk > 0) chunk = std::min(chunk, max_chunk);
  chunk = std::min(chunk, nprob);

  double *G = nullptr, *A = nullptr, *W = nullptr, *T = nullptr, *Dinv = nullptr, *u = nullptr;
  int *dinfo = nullptr;
  DevScope sc(st);
  GP_TRY(sc.alloc(&G, chunk * mp * Kcap));
  GP_TRY(sc.alloc(&A, chunk * mp * mp));
  GP_TRY(sc.alloc(&W, chunk * mp * mp));
  GP_TRY(sc.alloc(&T, chunk * mp * mp));
  GP_TRY(sc.alloc(&Dinv, chunk * mp * CV_NB));
  GP_TRY(sc.alloc(&u, chunk * mp));
  GP_TRY(sc.alloc(&dinfo, nprob));
  GP_HIP(hipMemsetAsync(dinfo, 0, sizeof(int) * (size_t)nprob, st));

  CvChunk c;
  c.Wt = m->Wt; c.alpha = m->alpha; c.jit = m->cv_jit; c.y = dy; c.idx = didx; c.foff = dfoff;
  c.G = G; c.A = A; c.W = W; c.u = u; c.mean = dmean; c.var = dvar;
  c.Npad = m->Npad; c.Kcap = Kcap; c.mp = mp; c.N = N; c.k = k;
  for (int64_t q0 = 0; q0 < nprob; q0 += chunk) {
    const int nb = (int)std::min(chunk, nprob - q0);
    c.q0 = (int)q0;
    hipLaunchKernelGGL(cv_gather_kernel, dim3((unsigned)mp, (unsigned)nb), dim3(256), 0, st, c);
    GP_HIP(hipGetLastError());
    // the tiles above the diagonal are never written by the SYRK: zero, like everything the solve may read
    GP_HIP(hipMemsetAsync(A, 0, sizeof(double) * (size_t)(nb * mp * mp), st));
    // A_II = G G^T, one batched launch per fold of the chunk (its K range starts at the fold's first point)
    for (int z0 = 0; z0 < nb;) {
      const int f = (int)((q0 + z0) / k);
      const int z1 = std::min<int>(nb, (int)((int64_t)(f + 1) * k - q0));
      GemmArgs g;
      g.A = G + (int64_t)z0 * mp * Kcap; g.lda = Kcap; g.strideA = mp * Kcap;
      g.B = g.A; g.ldb = Kcap; g.strideB = mp * Kcap;
      g.C = A + (int64_t)z0 * mp * mp; g.ldc = mp; g.strideC = mp * mp;
      g.M = (int)mp; g.N = (int)mp; g.K = (int)round_up(N - hr0[f], 16);
      g.lower_only = 1;
      GP_TRY(launch_gemm(g, false, false, z1 - z0, st));
      z0 = z1;
    }
    hipLaunchKernelGGL(cv_pad_diag_kernel, dim3((unsigned)nb), dim3(64), 0, st, c);
    GP_HIP(hipGetLastError());
    GP_TRY(device_cholesky_blocked(A, mp, Dinv, dinfo + q0, st, nb));
    GP_TRY(device_trtri_blocked(A, mp, Dinv, W, T, st, nb, true));
    hipLaunchKernelGGL(cv_u_kernel, dim3((unsigned)(mp / 4), (unsigned)nb), dim3(256), 0, st, c);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(cv_out_kernel, dim3((unsigned)((mp + 255) / 256), (unsigned)nb), dim3(256), 0, st, c);
    GP_HIP(hipGetLastError());
  }
  std::vector<int> info((size_t)nprob);
  GP_TRY(sc.download(info.data(), dinfo, nprob));
  GP_HIP(hipStreamSynchronize(st));
  for (int64_t q = 0; q < nprob; ++q)
    if (info[q] != 0) {
      set_error("cross_validate: A_II of fold %lld, PC %lld is not positive definite (pivot %d)", (long long)(q / k),
                (long long)(q % k), info[q]);
      return GPEMU_ERR_STATE;
    }
  return GPEMU_OK;
}

int launch_cv_backproject(gpemu_model *m, const double *dmean, const double *dvar, double *dcv, double *dvo) {
  if (!dcv && !dvo) return GPEMU_OK;
  hipLaunchKernelGGL(cv_backproject_kernel, dim3((unsigned)((m->F + 255) / 256), (unsigned)m->N), dim3(256), 0, m->stream,
                     dmean, dvar, m->comp, m->smean, m->sscale, m->cunexpl, (int)m->k, (int)m->F, dcv, dvo);
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

}  // namespace gpemu
