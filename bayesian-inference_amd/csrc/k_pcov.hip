// Joint predictive covariance of the PCs' GPs between query points, and draws from it (gpemu_gp_predict_cov,
// gpemu_gp_sample).  skl _gpr.py:367-469 (predict(X, return_cov=True)) and 498-531 (sample_y), with
// normalize_y = False as the project fits:
//   cov_p(X1, X2) = kernel_p(X1, X2) - V1^T V2,   V = W_p K_p(X_train, X)^T,   W_p = L_p^-1 (resident: Wt = W^T)
//   symmetric form (X2 = X1): kernel_p(X1) carries the White noise on the diagonal (only there), and the constant
//   everywhere; the two-set form carries no noise.  No clipping (skl clips only the return_std variance).
// Per chunk of PCs and of columns of X2 (both sized from the workspace):
//   kmat    K(A rows, B rows) per PC from the raw coordinates (direct distance, library exp / Bessel): the
//           train x query blocks KT = K(X_train, X)^T and the query x query block of C
//   V       V = W KT on the matrix cores (launch_gemm; k_to_m: the zero tiles of the triangle are skipped)
//   C       C = K12 - V1^T V2 (launch_gemm, alpha = -1, beta = 1); symmetric form: the lower tiles only, each element
//           then stored to both triangles, so that the output is symmetric bit for bit
// Draws: C_p + tau_p I = Lc Lc^T (device_cholesky_blocked, batched over PCs), Y_p = Lc Z_p (triangular GEMM), + mean.
// Every element's sums run in one fixed order whatever the chunking: the results do not depend on the workspace.
#include "internal.h"
#include "gemm.h"
#include "pcov_dev.h"

namespace gpemu {

// blockDim (64, 4): x = column (coalesced stores), 4 rows per thread (y, y + 4, ..); grid (cols / 64, rows / 16, PCs)
template <int KIND, int DP>
__global__ __launch_bounds__(256) void pcov_kmat_kernel(KmatArgs g) {
  const int z = blockIdx.z, p = g.p0 + z;
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t bi = g.b0 + c;
  double inv[DP], xb[DP];
#pragma unroll
  for (int dd = 0; dd < DP; ++dd) {
    inv[dd] = 1.0 / g.ls[(int64_t)p * g.dp + dd];
    xb[dd] = (dd < g.d && bi < g.nb) ? g.B[bi * g.sb + dd] : 0.0;
  }
  const double cst = g.constv[p];
  double *o = g.out + (int64_t)z * g.strideo;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = (int64_t)blockIdx.y * 16 + threadIdx.y + 4 * i;
    const int64_t ai = g.a0 + r;
    double v = 0.0;
    if (ai < g.na && bi < g.nb) {
      if (g.sym && ai == bi) {
        v = g.kdiag[p];
      } else {
        v = kmat_value<KIND, DP>(g.A + ai * g.sa, xb, inv, g.d, g.mn, cst);
      }
    }
    o[r * g.ldo + c] = v;
  }
}

int launch_kmat(const gpemu_model *m, KmatArgs g, int npc, hipStream_t st) {
  g.ls = m->ls; g.constv = m->constv; g.kdiag = m->kdiag; g.dp = m->dp; g.d = (int)m->d;
  if (kstar_kind(m) == 4) g.mn = matern_nu_constants(m->nu);
  dim3 grid((unsigned)(g.cols / 64), (unsigned)(g.rows / 16), (unsigned)npc), block(64, 4);
  GP_TRY(with_base_kind(kstar_kind(m), [&](auto kd) {
    constexpr int K = decltype(kd)::value;
    if (m->dp == DPAD) hipLaunchKernelGGL((pcov_kmat_kernel<K, DPAD>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((pcov_kmat_kernel<K, DPAD_WIDE>), grid, block, 0, st, g);
    return GPEMU_OK;
  }));
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

// V[z] = W_p KT[z]  (pcov_dev.h)
int launch_v(const gpemu_model *m, int p0, int npc, const double *KT, double *V, int64_t N64, int64_t ncols,
             hipStream_t st, int64_t strideV) {
  GemmArgs g;
  g.A = m->Wt + (int64_t)p0 * m->Npad * m->Npad; g.lda = m->Npad; g.strideA = m->Npad * m->Npad;   // [k][m]: W^T
  g.B = KT; g.ldb = ncols; g.strideB = N64 * ncols;
  g.C = V; g.ldc = ncols; g.strideC = strideV ? strideV : N64 * ncols;
  g.M = (int)N64; g.N = (int)ncols; g.K = (int)N64;
  g.k_to_m = 1;
  return launch_gemm(g, true, true, npc, st);
}

// out[p][a][b] from the chunk Cc[z][r][c] (a = r0 + r, b = c0 + c); sym: the lower triangle, stored to both
struct StoreArgs {
  const double *Cc = nullptr;
  int64_t ldc = 0, stridec = 0, rows = 0, cols = 0, r0 = 0, c0 = 0, M1 = 0, M2 = 0;
  double *out = nullptr;
  int p0 = 0, sym = 0;
};
__global__ __launch_bounds__(256) void pcov_store_kernel(StoreArgs s) {
  const int z = blockIdx.z;
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x, b = s.c0 + c;
  if (c >= s.cols || b >= s.M2) return;
  const double *src = s.Cc + (int64_t)z * s.stridec;
  double *o = s.out + (int64_t)(s.p0 + z) * s.M1 * s.M2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = (int64_t)blockIdx.y * 16 + threadIdx.y + 4 * i, a = s.r0 + r;
    if (r >= s.rows || a >= s.M1) continue;
    if (s.sym && a < b) continue;
    const double v = src[r * s.ldc + c];
    o[a * s.M2 + b] = v;
    if (s.sym) o[b * s.M2 + a] = v;
  }
}

// the chunk sizes: PCs per chunk and columns of X2 per chunk (a multiple of 64), within `budget` bytes
static bool pcov_plan(int64_t k, int64_t N64, int64_t M1p, int64_t M2p, bool sym, int64_t budget, int &pc, int64_t &mc) {
  for (pc = (int)k; pc >= 1; --pc) {
    const int64_t fixed = (int64_t)pc * 2 * N64 * M1p * 8;                          // KT1, V1
    const int64_t per_col = (int64_t)pc * (M1p + (sym ? 0 : 2 * N64)) * 8;         // Cc (+ KT2, V2)
    if (budget <= fixed) continue;
    mc = (budget - fixed) / per_col / PC_NB * PC_NB;
    if (mc > M2p) mc = M2p;
    if (mc >= PC_NB) return true;
  }
  return false;
}

// the workspace of one call: auto = a quarter of the free device memory, at most 8 GiB (as k_cv.hip)
static int pcov_budget(int64_t workspace_bytes, int64_t &budget, bool &automatic) {
  automatic = workspace_bytes <= 0;
  if (!automatic) { budget = workspace_bytes; return GPEMU_OK; }
  size_t fb = 0, tb = 0;
  GP_HIP(hipMemGetInfo(&fb, &tb));
  budget = std::min<int64_t>((int64_t)(fb / 4), (int64_t)8 << 30);
  return GPEMU_OK;
}

// dX1 [M1][d], dX2 [M2][d] or null (symmetric form) -> dcov [k][M1][M2]; everything on st (asynchronous)
int predict_cov(gpemu_model *m, int64_t M1, const double *dX1, int64_t M2, const double *dX2, int64_t workspace_bytes,
                double *dcov, hipStream_t st) {
  const bool sym = dX2 == nullptr;
  if (sym) M2 = M1;
  const int64_t N = m->N, k = m->k, N64 = round_up(N, PC_NB), Kc = round_up(N, 16);
  const int64_t M1p = round_up(M1, PC_NB), M2p = round_up(M2, PC_NB);
  int64_t budget = 0;
  bool automatic = false;
  GP_TRY(pcov_budget(workspace_bytes, budget, automatic));
  int pc = 0;
  int64_t mc = 0;
  if (!pcov_plan(k, N64, M1p, M2p, sym, budget, pc, mc)) {
    const int64_t need = 2 * N64 * M1p * 8 + (M1p + (sym ? 0 : 2 * N64)) * 8 * PC_NB;
    if (automatic)
      set_error("bad argument: predict_cov: the device is too full for one column tile of one PC (%lld bytes needed, "
                "%lld available)", (long long)need, (long long)budget);
    else
      set_error("bad argument: predict_cov: workspace_bytes = %lld is too small for one column tile of one PC "
                "(%lld bytes needed)", (long long)workspace_bytes, (long long)need);
    return GPEMU_ERR_ARG;
  }
  DevScope sc(st);
  double *KT1 = nullptr, *V1 = nullptr, *KT2 = nullptr, *V2 = nullptr, *Cc = nullptr;
  const int rc = [&]() -> int {
    GP_TRY(sc.alloc(&KT1, (int64_t)pc * N64 * M1p));
    GP_TRY(sc.alloc(&V1, (int64_t)pc * N64 * M1p));
    if (!sym) GP_TRY(sc.alloc(&KT2, (int64_t)pc * N64 * mc));
    if (!sym) GP_TRY(sc.alloc(&V2, (int64_t)pc * N64 * mc));
    return sc.alloc(&Cc, (int64_t)pc * M1p * mc);
  }();
  if (rc != GPEMU_OK) {
    if (automatic) {   // the free memory went elsewhere between the query and the allocation: the allocation's own
      const std::string why = gpemu_last_error();   // code (no argument of the caller's is at fault), with the reason
      set_error("predict_cov: the device is too full for the workspace (%s)", why.c_str());
    }
    return rc;
  }
  const int d = (int)m->d;
  for (int p0 = 0; p0 < (int)k; p0 += pc) {
    const int np = std::min<int>(pc, (int)k - p0);
    KmatArgs g;
    g.A = m->Xtr; g.sa = m->dp; g.na = N; g.B = dX1; g.sb = d; g.nb = M1; g.p0 = p0;
    g.out = KT1; g.ldo = M1p; g.strideo = N64 * M1p; g.rows = N64; g.cols = M1p;
    GP_TRY(launch_kmat(m, g, np, st));
    GP_TRY(launch_v(m, p0, np, KT1, V1, N64, M1p, st));
    for (int64_t c0 = 0; c0 < M2p; c0 += mc) {
      const int64_t nc = std::min(mc, M2p - c0);
      const int64_t r0 = sym ? c0 : 0;               // symmetric form: rows from the chunk's first column down
      const int64_t nr = M1p - r0;
      // K12 into Cc
      KmatArgs h;
      h.A = dX1; h.sa = d; h.na = M1; h.a0 = r0;
      h.B = sym ? dX1 : dX2; h.sb = d; h.nb = M2; h.b0 = c0;
      h.out = Cc; h.ldo = nc; h.strideo = M1p * nc; h.rows = nr; h.cols = nc; h.p0 = p0; h.sym = sym ? 1 : 0;
      GP_TRY(launch_kmat(m, h, np, st));
      const double *B = V1 + c0;
      int64_t ldb = M1p, strideB = N64 * M1p;
      if (!sym) {
        KmatArgs t;
        t.A = m->Xtr; t.sa = m->dp; t.na = N; t.B = dX2; t.sb = d; t.nb = M2; t.b0 = c0; t.p0 = p0;
        t.out = KT2; t.ldo = nc; t.strideo = N64 * nc; t.rows = N64; t.cols = nc;
        GP_TRY(launch_kmat(m, t, np, st));
        GP_TRY(launch_v(m, p0, np, KT2, V2, N64, nc, st));
        B = V2; ldb = nc; strideB = N64 * nc;
      }
      // Cc = K12 - V1[:, r0 ..]^T V2
      GemmArgs c;
      c.A = V1 + r0; c.lda = M1p; c.strideA = N64 * M1p;
      c.B = B; c.ldb = ldb; c.strideB = strideB;
      c.C = Cc; c.ldc = nc; c.strideC = M1p * nc;
      c.M = (int)nr; c.N = (int)nc; c.K = (int)Kc;
      c.alpha = -1.0; c.beta = 1.0;
      c.lower_only = sym ? 1 : 0;
      GP_TRY(launch_gemm(c, true, true, np, st));
      StoreArgs s;
      s.Cc = Cc; s.ldc = nc; s.stridec = M1p * nc; s.rows = nr; s.cols = nc; s.r0 = r0; s.c0 = c0;
      s.M1 = M1; s.M2 = M2; s.out = dcov; s.p0 = p0; s.sym = sym ? 1 : 0;
      hipLaunchKernelGGL(pcov_store_kernel, dim3((unsigned)(nc / 64), (unsigned)(nr / 16), (unsigned)np), dim3(64, 4), 0,
                         st, s);
      GP_HIP(hipGetLastError());
    }
  }
  // the workspace is freed on return: its last readers must be done
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

// ---- draws --------------------------------------------------------------------------------------------------------
struct DrawArgs {
  const double *cov = nullptr;   // [k][M][M]
  const double *z = nullptr;     // [k][M][n]
  const double *mean = nullptr;  // [M][k]
  const int *pc_of = nullptr;    // [slots] PC of each batch slot
  const double *tau = nullptr;   // [slots]
  const int *ok = nullptr;       // [slots] factor found: store the draws
  double *A = nullptr;           // [slots][Mp][Mp]
  double *Z = nullptr;           // [slots][Mp][np]
  double *Y = nullptr;           // [slots][Mp][np]
  double *out = nullptr;         // [k][M][n]
  int64_t M = 0, n = 0, Mp = 0, np = 0, k = 0;
};

// A = lower(C_p) + tau I, zero above the diagonal, identity on the padded diagonal; Z the slot's normals, padded
__global__ __launch_bounds__(256) void pcov_chol_setup_kernel(DrawArgs a) {
  const int s = blockIdx.y;
  const int64_t r = blockIdx.x;
  const int p = a.pc_of[s];
  const double tau = a.tau[s];
  double *Ar = a.A + ((int64_t)s * a.Mp + r) * a.Mp;
  const double *Cr = a.cov + ((int64_t)p * a.M + r) * a.M;
  for (int64_t c = threadIdx.x; c < a.Mp; c += 256) {
    double v = 0.0;
    if (r < a.M && c < r) v = Cr[c];
    else if (c == r) v = r < a.M ? Cr[c] + tau : 1.0;
    Ar[c] = v;
  }
  double *Zr = a.Z + ((int64_t)s * a.Mp + r) * a.np;
  const double *zr = a.z + ((int64_t)p * a.M + r) * a.n;
  for (int64_t c = threadIdx.x; c < a.np; c += 256) Zr[c] = (r < a.M && c < a.n) ? zr[c] : 0.0;
}

// the factor's strict upper triangle to zero (device_cholesky_blocked leaves its diagonal blocks' scratch there, and the
// triangular GEMM reads whole 64 x 64 tiles)
__global__ __launch_bounds__(256) void pcov_zero_upper_kernel(double *A, int64_t Mp) {
  const int64_t r = blockIdx.x;
  double *Ar = A + ((int64_t)blockIdx.y * Mp + r) * Mp;
  for (int64_t c = r + 1 + threadIdx.x; c < Mp; c += 256) Ar[c] = 0.0;
}

// out[p][i][j] = mean_p(x_i) + Y[i][j] for the slots whose factor was found
__global__ __launch_bounds__(256) void pcov_draw_store_kernel(DrawArgs a) {
  const int s = blockIdx.y;
  const int64_t i = blockIdx.x;
  if (!a.ok[s]) return;
  const int p = a.pc_of[s];
  const double mu = a.mean[i * a.k + p];
  const double *Yr = a.Y + ((int64_t)s * a.Mp + i) * a.np;
  double *o = a.out + ((int64_t)p * a.M + i) * a.n;
  for (int64_t j = threadIdx.x; j < a.n; j += 256) o[j] = mu + Yr[j];
}

constexpr int PC_LADDER = 7;   // tau = 1e-12 mean(diag C) 10^i, i = 0 .. 6, after tau = 0

// dcov [k][M][M] (symmetric form), dmean [M][k], dz [k][M][n] -> dout [k][M][n], tau_out[k] (host).  Returns p + 1 for
// the first PC whose ladder is exhausted (its draws are not written), after every other PC has been drawn.
int sample_from_cov(gpemu_model *m, int64_t M, int64_t n, const double *dcov, const double *dmean, const double *dz,
                    double *dout, double *tau_out, hipStream_t st) {
  const int k = (int)m->k;
  const int64_t Mp = round_up(M, PC_NB), np = round_up(n, PC_NB);
  // mean of each PC's diagonal, summed in index order on the host
  std::vector<double> diag((size_t)(k * M)), dmeanv((size_t)k);
  for (int p = 0; p < k; ++p)
    GP_HIP(hipMemcpy2DAsync(diag.data() + (size_t)p * M, sizeof(double), dcov + (int64_t)p * M * M,
                            sizeof(double) * (size_t)(M + 1), sizeof(double), (size_t)M, hipMemcpyDeviceToHost, st));
  GP_HIP(hipStreamSynchronize(st));
  for (int p = 0; p < k; ++p) {
    double s = 0.0;
    for (int64_t i = 0; i < M; ++i) s += diag[(size_t)(p * M + i)];
    dmeanv[(size_t)p] = s / (double)M;
  }
  int64_t budget = 0;
  bool automatic = false;
  GP_TRY(pcov_budget(0, budget, automatic));
  const int64_t per = (Mp * Mp + Mp * PC_NB + 2 * Mp * np) * 8;
  if (budget < per) {
    set_error("bad argument: sample: the device is too full for the factor of one PC (%lld bytes needed, %lld available)",
              (long long)per, (long long)budget);
    return GPEMU_ERR_ARG;
  }
  const int slots = (int)std::min<int64_t>(k, std::max<int64_t>(1, std::min<int64_t>(budget / per, 16384 * 64 / Mp)));
  DevScope sc(st);
  DrawArgs a;
  double *A = nullptr, *Dinv = nullptr, *Z = nullptr, *Y = nullptr, *tau = nullptr;
  int *pc_of = nullptr, *ok = nullptr, *dinfo = nullptr;
  GP_TRY(sc.alloc(&A, (int64_t)slots * Mp * Mp));
  GP_TRY(sc.alloc(&Dinv, (int64_t)slots * Mp * PC_NB));
  GP_TRY(sc.alloc(&Z, (int64_t)slots * Mp * np));
  GP_TRY(sc.alloc(&Y, (int64_t)slots * Mp * np));
  GP_TRY(sc.alloc(&tau, slots));
  GP_TRY(sc.alloc(&pc_of, slots));
  GP_TRY(sc.alloc(&ok, slots));
  GP_TRY(sc.alloc(&dinfo, slots));
  a.cov = dcov; a.z = dz; a.mean = dmean; a.pc_of = pc_of; a.tau = tau; a.ok = ok;
  a.A = A; a.Z = Z; a.Y = Y; a.out = dout; a.M = M; a.n = n; a.Mp = Mp; a.np = np; a.k = k;
  std::vector<int> todo;   // PCs without a factor yet
  std::vector<int> rung((size_t)k, -1);
  for (int p = 0; p < k; ++p) todo.push_back(p);
  int first_fail = 0;
  while (!todo.empty()) {
    const int ns = (int)std::min<size_t>((size_t)slots, todo.size());
    std::vector<int> hpc(todo.begin(), todo.begin() + ns), hinfo((size_t)ns, 0), hok((size_t)ns, 0);
    std::vector<double> htau((size_t)ns);
    for (int s = 0; s < ns; ++s) {
      const int p = hpc[(size_t)s], i = rung[(size_t)p];
      const double md = dmeanv[(size_t)p] > 0.0 ? dmeanv[(size_t)p] : 1.0;
      htau[(size_t)s] = i < 0 ? 0.0 : 1e-12 * md * std::pow(10.0, (double)i);
    }
    GP_HIP(hipMemcpyAsync(pc_of, hpc.data(), sizeof(int) * (size_t)ns, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(tau, htau.data(), sizeof(double) * (size_t)ns, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemsetAsync(dinfo, 0, sizeof(int) * (size_t)ns, st));
    hipLaunchKernelGGL(pcov_chol_setup_kernel, dim3((unsigned)Mp, (unsigned)ns), dim3(256), 0, st, a);
    GP_HIP(hipGetLastError());
    GP_TRY(device_cholesky_blocked(A, Mp, Dinv, dinfo, st, ns));
    GP_HIP(hipMemcpyAsync(hinfo.data(), dinfo, sizeof(int) * (size_t)ns, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    std::vector<int> next;
    for (int s = 0; s < ns; ++s) {
      const int p = hpc[(size_t)s];
      if (hinfo[(size_t)s] == 0) {
        hok[(size_t)s] = 1;
        tau_out[p] = htau[(size_t)s];
      } else if (++rung[(size_t)p] < PC_LADDER) {
        next.push_back(p);
      } else {
        tau_out[p] = NAN;
        if (!first_fail || p + 1 < first_fail) first_fail = p + 1;
      }
    }
    GP_HIP(hipMemcpyAsync(ok, hok.data(), sizeof(int) * (size_t)ns, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pcov_zero_upper_kernel, dim3((unsigned)Mp, (unsigned)ns), dim3(256), 0, st, A, Mp);
    GP_HIP(hipGetLastError());
    // Y = Lc Z: Lc lower triangular (k_to_m: the K range of a row tile ends at its last row)
    GemmArgs g;
    g.A = A; g.lda = Mp; g.strideA = Mp * Mp;
    g.B = Z; g.ldb = np; g.strideB = Mp * np;
    g.C = Y; g.ldc = np; g.strideC = Mp * np;
    g.M = (int)Mp; g.N = (int)np; g.K = (int)Mp;
    g.k_to_m = 1;
    GP_TRY(launch_gemm(g, false, true, ns, st));
    hipLaunchKernelGGL(pcov_draw_store_kernel, dim3((unsigned)M, (unsigned)ns), dim3(256), 0, st, a);
    GP_HIP(hipGetLastError());
    GP_HIP(hipStreamSynchronize(st));   // hok / htau / the slots are reused by the next round
    next.insert(next.end(), todo.begin() + ns, todo.end());
    todo.swap(next);
  }
  if (first_fail) {
    set_error("sample: C + tau I of PC %d is not positive definite up to tau = 1e-6 mean(diag C)", first_fail - 1);
    return first_fail;
  }
  return GPEMU_OK;
}

}  // namespace gpemu
