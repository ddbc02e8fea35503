// Sequential design by integrated variance reduction (gpemu_design_*): where should the model be run next?
// For PC p with the two-set predictive covariance c_p (k_pcov.hip; no noise), reference rows x_s with weights omega_s
// (sum 1) and candidates x_c:
//   IV_p = sum_s omega_s c_p(s, s)     den_p(c) = c_p(c, c) + tau_p
//   score(c) = sum_p w_p [sum_s omega_s c_p(s, c)^2] / den_p(c)      (a PC with den <= min_variance kernel_.diag_p: 0)
// After j picks c_p^(j)(s, c) = K(s, c) - V_s^T V_c - sum_{i<j} u_i(s) u_i(c): the picks' columns u_i are rows appended
// to the two GEMM operands V1' [N64 + picks][S64] and V2' [N64 + picks][M64] (k-major), which the handle keeps.
//   V        kmat + launch_gemm, exactly as k_pcov.hip (pcov_dev.h), into the operands; the spare rows zero
//   den0     column sums of squares of V in row order: c(s, s) (for IV_0) and den_0(c) = 1 + const - |V_c|^2 + tau
//   wsum     IV_p = sum_s omega_s c(s, s), later IV_p -= sum_s omega_s u(s)^2: lane-strided sums, then tree A (wg_dev.h)
//   score    per PC a 64 x 64 tile of V1'^T V2' on the matrix cores; the epilogue forms K(x_s, x_c) of each element from
//            the raw rows (kmat_value: the numerics of pcov_kmat_kernel), subtracts, squares, weights, and adds the 64
//            rows of the tile in a fixed order: one partial per (PC, row tile, candidate).  The S x M matrix never exists.
//   finish   per candidate: the row tiles' partials in index order, / den under the floor rule, * w_p, PCs in index order
//   column   for a pick c*: c^(j)(., c*) over the reference rows and the candidates (a dot product per column, rows in
//            index order), u = column / sqrt(den(c*)) into the spare row, den -= u^2
// No floating-point atomics; every sum's order depends on its indices only: the bits do not depend on the chunking.
#include <algorithm>

#include "internal.h"
#include "gemm.h"
#include "pcov_dev.h"
#include "rows_dev.h"
#include "wg_dev.h"

struct gpemu_design {
  gpemu_model *m = nullptr;
  int64_t S = 0, M = 0, Sp = 0, Mp = 0, N64 = 0, Kcap = 0, k = 0, max_picks = 0, n_picks = 0;
  int64_t mc = 0;              // candidates per chunk of partials (a multiple of 64)
  double *V1 = nullptr;        // [k][Kcap][Sp]  V of the reference rows, then the picks' u over them
  double *V2 = nullptr;        // [k][Kcap][Mp]  ... of the candidates
  double *Xref = nullptr;      // [Sp][d]  (padded rows = 0)
  double *Xcand = nullptr;     // [Mp][d]
  double *omega = nullptr;     // [Sp]     normalised weights (padding = 0)
  double *pcw = nullptr, *tau = nullptr, *floorv = nullptr, *dstar = nullptr, *iv = nullptr;   // [k]
  double *den = nullptr;       // [k][Mp]
  double *cdiag = nullptr;     // [k][Sp]  c(s, s) of the create call
  double *part = nullptr;      // [k][Sp / 64][mc]
  double *score = nullptr;     // [Mp]
  double *score_pc = nullptr;  // [k][Mp]
};

namespace gpemu {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

static inline void design_path_count(int path) { count_path(PATHS_DESIGN, path); }   // enum gpemu_design_path

// ---- column sums of squares: c(x, x) = 1 + const - |V_x|^2 (+ add[p]) ------------------------------------------------
// grid (cols / 256 rounded up, k); V [k][Kcap][ld]: rows [0, nrows) in index order
__global__ __launch_bounds__(256) void design_den0_kernel(const double *__restrict__ V, int64_t Kcap, int64_t ld,
                                                          int64_t nrows, const double *__restrict__ constv,
                                                          const double *__restrict__ add, double *__restrict__ out) {
  const int p = blockIdx.y;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= ld) return;
  const double *v = V + (int64_t)p * Kcap * ld + c;
  double s = 0.0;
  for (int64_t r = 0; r < nrows; ++r) {
    const double x = v[r * ld];
    s = fma(x, x, s);
  }
  double o = (1.0 + constv[p]) - s;
  if (add) o += add[p];
  out[(int64_t)p * ld + c] = o;
}

// ---- iv[p] = sum_s omega_s v_s (square = 0) or iv[p] -= sum_s omega_s v_s^2 (square = 1); grid k ----------------------
__global__ __launch_bounds__(256) void design_wsum_kernel(const double *__restrict__ vals, int64_t stride, int64_t Sp,
                                                          const double *__restrict__ omega, int square,
                                                          double *__restrict__ iv) {
  __shared__ double red[256];
  const int p = blockIdx.x, t = threadIdx.x;
  const double *v = vals + (int64_t)p * stride;
  double s = 0.0;
  for (int64_t i = t; i < Sp; i += 256) {
    const double x = v[i];
    s = fma(omega[i], square ? x * x : x, s);
  }
  s = wg_sum_a<256>(s, red);
  if (t == 0) iv[p] = square ? iv[p] - s : s;
}

// ---- the score kernel ----------------------------------------------------------------------------------------------
struct ScoreArgs {
  const double *V1 = nullptr, *V2 = nullptr;
  int64_t Sp = 0, Mp = 0, Kcap = 0, N64 = 0;
  int nk1 = 0, nk2 = 0;        // 16-row k-tiles of the rows [0, 16 nk1) (the training rows) and [N64, N64 + 16 nk2) (picks)
  const double *Xref = nullptr, *Xcand = nullptr, *omega = nullptr;
  int64_t S = 0, M = 0, c0 = 0, ldp = 0;   // c0: first candidate of the chunk; ldp: row length of part
  double *part = nullptr;      // [k][gridDim.y][ldp]
  const double *ls = nullptr, *constv = nullptr;
  int dp = DPAD, d = 1;
  MaternNu mn;
};

// grid (candidate tiles of the chunk, row tiles, PCs), 256 threads = 4 waves (2 x 2, 32 x 32 of the tile each): the
// schedule of gemm_f64_kernel<true, true, 2> (k-step 16, LDS double buffered, two register stages)
template <int KIND, int DP>
__global__ __launch_bounds__(256) void design_score_kernel(ScoreArgs g) {
  constexpr int T = 64, GK = 16, SK = T + 16, NST = T * GK / 2 / 256;
  __shared__ __attribute__((aligned(16))) double sA[2][GK * SK];
  __shared__ __attribute__((aligned(16))) double sB[2][GK * SK];
  const int z = blockIdx.z;
  const int64_t m0 = (int64_t)blockIdx.y * T, n0 = g.c0 + (int64_t)blockIdx.x * T;
  const double *A = g.V1 + (int64_t)z * g.Kcap * g.Sp + m0;
  const double *B = g.V2 + (int64_t)z * g.Kcap * g.Mp + n0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lk = lane >> 4;

  d2 ra0[NST], rb0[NST], ra1[NST], rb1[NST];
  auto gload = [&](int kt, d2 (&ra)[NST], d2 (&rb)[NST]) {
    const int64_t row0 = kt < g.nk1 ? (int64_t)kt * GK : g.N64 + (int64_t)(kt - g.nk1) * GK;
#pragma unroll
    for (int r = 0; r < NST; ++r) {
      const int idx = tid + 256 * r;
      const int64_t row = row0 + idx / (T / 2);
      const int col = 2 * (idx % (T / 2));
      ra[r] = *reinterpret_cast<const d2 *>(A + row * g.Sp + col);
      rb[r] = *reinterpret_cast<const d2 *>(B + row * g.Mp + col);
    }
  };
  auto sstore = [&](int buf, const d2 (&ra)[NST], const d2 (&rb)[NST]) {
#pragma unroll
    for (int r = 0; r < NST; ++r) {
      const int idx = tid + 256 * r;
      *reinterpret_cast<d2 *>(&sA[buf][(idx / (T / 2)) * SK + 2 * (idx % (T / 2))]) = ra[r];
      *reinterpret_cast<d2 *>(&sB[buf][(idx / (T / 2)) * SK + 2 * (idx % (T / 2))]) = rb[r];
    }
  };
  d4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};

  const int nk = g.nk1 + g.nk2;
  gload(0, ra0, rb0);
  if (1 < nk) gload(1, ra1, rb1);
  sstore(0, ra0, rb0);
  __syncthreads();
  auto ktile = [&](int kt, int buf, d2 (&ra_ld)[NST], d2 (&rb_ld)[NST], const d2 (&ra_nxt)[NST], const d2 (&rb_nxt)[NST]) {
    if (kt + 2 < nk) gload(kt + 2, ra_ld, rb_ld);
#pragma unroll
    for (int ks = 0; ks < GK / 4; ++ks) {
      double a[2], b[2];
      const int kk = ks * 4 + lk;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) a[mi] = sA[buf][kk * SK + wm * 32 + mi * 16 + lr];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) b[ni] = sB[buf][kk * SK + wn * 32 + ni * 16 + lr];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
    if (kt + 1 < nk) sstore(buf ^ 1, ra_nxt, rb_nxt);
    __syncthreads();
  };
  for (int kt = 0; kt < nk; kt += 2) {
    ktile(kt, 0, ra0, rb0, ra1, rb1);
    if (kt + 1 < nk) ktile(kt + 1, 1, ra1, rb1, ra0, rb0);
  }

  // the epilogue: the operand tiles are done with (the last k-tile ended in a barrier); their LDS holds the tile's raw
  // reference rows, 1 / ls, the weights and the partial sums of the reduction
  double *sX = &sA[0][0];          // [64][DP]
  double *sInv = &sB[0][0];        // [DP]
  double *sOm = sInv + 16;         // [64]
  double *sRed = sInv + 128;       // [8][64]
  const int p = z;
  for (int idx = tid; idx < T * DP; idx += 256) {
    const int r = idx / DP, dd = idx % DP;
    const int64_t s = m0 + r;
    sX[idx] = (dd < g.d && s < g.S) ? g.Xref[s * g.d + dd] : 0.0;
  }
  if (tid < DP) sInv[tid] = 1.0 / g.ls[(int64_t)p * g.dp + tid];
  if (tid < T) sOm[tid] = g.omega[m0 + tid];
  __syncthreads();
  const double cst = g.constv[p];
  // D[reg] is row (lane >> 4) + 4 * reg, column lane & 15 of each 16 x 16 tile
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = wn * 32 + ni * 16 + lr;
    const int64_t c = n0 + col;
    double xc[DP];
#pragma unroll
    for (int dd = 0; dd < DP; ++dd) xc[dd] = (dd < g.d && c < g.M) ? g.Xcand[c * g.d + dd] : 0.0;
    double sum = 0.0;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * 32 + mi * 16 + lk + 4 * r;
        const double kv = kmat_value<KIND, DP>(sX + row * DP, xc, sInv, g.d, g.mn, cst);
        const double e = kv - acc[mi][ni][r];
        sum = fma(sOm[row], e * e, sum);
      }
    }
    sRed[(wm * 4 + lk) * T + col] = sum;
  }
  __syncthreads();
  if (tid < T) {
    double tot = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) tot += sRed[j * T + tid];
    g.part[((int64_t)z * gridDim.y + blockIdx.y) * g.ldp + (int64_t)blockIdx.x * T + tid] = tot;
  }
}

// ---- per candidate: partials -> score --------------------------------------------------------------------------------
struct FinishArgs {
  const double *part = nullptr;    // [k][nrt][ldp]
  int64_t ldp = 0, nc = 0, c0 = 0, M = 0, Mp = 0;
  int nrt = 0, k = 0;
  const double *den = nullptr, *pcw = nullptr, *floorv = nullptr;
  double *score = nullptr, *score_pc = nullptr;
};
__global__ __launch_bounds__(256) void design_finish_kernel(FinishArgs f) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= f.nc) return;
  const int64_t c = f.c0 + i;
  double tot = 0.0;
  for (int p = 0; p < f.k; ++p) {
    double num = 0.0;
    const double *pp = f.part + (int64_t)p * f.nrt * f.ldp + i;
    for (int t = 0; t < f.nrt; ++t) num += pp[(int64_t)t * f.ldp];
    const double dn = f.den[(int64_t)p * f.Mp + c];
    const double v = (c < f.M && dn > f.floorv[p]) ? f.pcw[p] * (num / dn) : 0.0;
    f.score_pc[(int64_t)p * f.Mp + c] = v;
    tot += v;
  }
  f.score[c] = tot;
}

// ---- conditioning on a pick ------------------------------------------------------------------------------------------
__global__ void design_pick_kernel(const double *__restrict__ den, int64_t Mp, int64_t cstar, int k,
                                   double *__restrict__ dstar) {
  const int p = threadIdx.x;
  if (p < k) dstar[p] = den[(int64_t)p * Mp + cstar];
}

struct ColumnArgs {
  double *V1 = nullptr, *V2 = nullptr;
  int64_t Sp = 0, Mp = 0, Kcap = 0, N64 = 0, S = 0, M = 0, cstar = 0;
  int j = 0;                       // picks so far: u goes to row N64 + j
  const double *Xref = nullptr, *Xcand = nullptr;
  const double *dstar = nullptr, *floorv = nullptr;
  double *den = nullptr;
  const double *ls = nullptr, *constv = nullptr;
  int dp = DPAD, d = 1;
  MaternNu mn;
};
// grid ((Sp + Mp) / 256 rounded up, k): column i < Sp is reference row i, else candidate i - Sp
template <int KIND, int DP>
__global__ __launch_bounds__(256) void design_column_kernel(ColumnArgs g) {
  const int p = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.Sp + g.Mp) return;
  const bool ref = i < g.Sp;
  const int64_t col = ref ? i : i - g.Sp, ld = ref ? g.Sp : g.Mp, n = ref ? g.S : g.M;
  double *V = (ref ? g.V1 : g.V2) + (int64_t)p * g.Kcap * ld;
  const double *Vs = g.V2 + (int64_t)p * g.Kcap * g.Mp + g.cstar;
  const int64_t urow = g.N64 + g.j;
  double u = 0.0;
  const double ds = g.dstar[p];
  if (col < n && ds > g.floorv[p]) {
    double dot = 0.0;
    for (int64_t r = 0; r < g.N64; ++r) dot = fma(V[r * ld + col], Vs[r * g.Mp], dot);
    for (int64_t r = g.N64; r < urow; ++r) dot = fma(V[r * ld + col], Vs[r * g.Mp], dot);
    double inv[DP], xb[DP];
#pragma unroll
    for (int dd = 0; dd < DP; ++dd) {
      inv[dd] = 1.0 / g.ls[(int64_t)p * g.dp + dd];
      xb[dd] = dd < g.d ? g.Xcand[g.cstar * g.d + dd] : 0.0;
    }
    const double *a = (ref ? g.Xref : g.Xcand) + col * g.d;
    const double kv = kmat_value<KIND, DP>(a, xb, inv, g.d, g.mn, g.constv[p]);
    u = (kv - dot) / sqrt(ds);
  }
  V[urow * ld + col] = u;
  if (!ref) g.den[(int64_t)p * g.Mp + col] -= u * u;
}

// the launch of a kernel template by the model's base kind and padded width
template <class Fn>
static int with_kind_dp(const gpemu_model *m, Fn &&fn) {
  return with_base_kind(kstar_kind(m), [&](auto kd) {
    constexpr int K = decltype(kd)::value;
    if (m->dp == DPAD) return fn(std::integral_constant<int, K>{}, std::integral_constant<int, DPAD>{});
    return fn(std::integral_constant<int, K>{}, std::integral_constant<int, DPAD_WIDE>{});
  });
}

static int64_t design_operand_bytes(int64_t k, int64_t Kcap, int64_t Sp, int64_t Mp) {
  return (k * Kcap * (Sp + Mp) + k * Sp + 2 * k * Mp + Sp + Mp) * 8;   // V1, V2, cdiag, den, score_pc, omega, score
}

static void design_free(gpemu_design *h) {
  dev_free(h->V1); dev_free(h->V2); dev_free(h->Xref); dev_free(h->Xcand); dev_free(h->omega); dev_free(h->pcw);
  dev_free(h->tau); dev_free(h->floorv); dev_free(h->dstar); dev_free(h->iv); dev_free(h->den); dev_free(h->cdiag);
  dev_free(h->part); dev_free(h->score); dev_free(h->score_pc);
  delete h;
}

struct DesignSpec {
  int64_t S = 0, M = 0, max_picks = 0, workspace_bytes = 0;
  const double *w_ref = nullptr, *pc_weight = nullptr, *tau = nullptr;
  double min_variance = 0.0;
};

static bool finite_nonneg(const double *x, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!(std::isfinite(x[i]) && x[i] >= 0.0)) return false;
  return true;
}

// what both create calls check before any launch
static int design_check(const gpemu_model *m, const DesignSpec &q) {
  GP_ARG(q.S >= 1 && q.S <= 4194240, "S must be in [1, 4194240]");
  GP_ARG(q.M >= 1 && q.M <= 4194240, "M must be in [1, 4194240]");
  GP_ARG(m->d <= 16, "d must be at most 16");
  GP_ARG(m->k <= 64, "k must be at most 64");
  GP_ARG(q.max_picks >= 0 && q.max_picks <= 256, "max_picks must be in [0, 256]");
  GP_ARG(std::isfinite(q.min_variance) && q.min_variance >= 0.0, "min_variance must be finite and >= 0");
  GP_ARG(q.workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_ARG(q.pc_weight && finite_nonneg(q.pc_weight, m->k), "pc_weight must be finite and >= 0");
  GP_ARG(!q.tau || finite_nonneg(q.tau, m->k), "tau must be finite and >= 0");
  if (q.w_ref) {
    GP_ARG(finite_nonneg(q.w_ref, q.S), "w_ref must be finite and >= 0");
    double s = 0.0;
    for (int64_t i = 0; i < q.S; ++i) s += q.w_ref[i];
    GP_ARG(s > 0.0 && std::isfinite(s), "w_ref must have a positive, finite sum");
  }
  return GPEMU_OK;
}

// the workspace the handle may use, or GPEMU_ERR_ARG where the operands and one tile of partials do not fit in it.  The
// create calls ask before they allocate anything: a handle that is refused costs no allocation
static int design_budget(const gpemu_model *m, const DesignSpec &q, int64_t *budget) {
  const int64_t S = q.S, M = q.M, k = m->k, d = m->d, N = m->N;
  const int64_t Sp = round_up(S, PC_NB), Mp = round_up(M, PC_NB), N64 = round_up(N, PC_NB);
  const int64_t Kcap = N64 + round_up(q.max_picks, 16), colsmax = std::max(Sp, Mp), nrt = Sp / PC_NB;
  GP_TRY(workspace_budget(q.workspace_bytes, budget));
  const int64_t fixed = design_operand_bytes(k, Kcap, Sp, Mp) + (Sp + Mp) * d * 8;
  const int64_t tile = std::max(k * nrt * PC_NB * 8, N64 * colsmax * 8);   // one tile of partials; the create call's KT
  if (*budget < fixed + tile) {
    set_error("bad argument: design: %lld bytes are needed for the operands and one tile of partials, %lld are %s",
              (long long)(fixed + tile), (long long)*budget, workspace_budget_name(q.workspace_bytes));
    return GPEMU_ERR_ARG;
  }
  return GPEMU_OK;
}

// the handle from checked arguments and device rows; the model's device is current
static int design_build(gpemu_design **out, gpemu_model *m, const DesignSpec &q, const RowsView &ref, const double *dXcand) {
  hipStream_t st = m->stream;
  const int64_t S = q.S, M = q.M, k = m->k, d = m->d, N = m->N;
  const int64_t Sp = round_up(S, PC_NB), Mp = round_up(M, PC_NB), N64 = round_up(N, PC_NB);
  const int64_t Kcap = N64 + round_up(q.max_picks, 16), colsmax = std::max(Sp, Mp), nrt = Sp / PC_NB;
  int64_t budget = 0;
  GP_TRY(design_budget(m, q, &budget));
  const int64_t fixed = design_operand_bytes(k, Kcap, Sp, Mp) + (Sp + Mp) * d * 8;
  gpemu_design *h = new gpemu_design();
  h->m = m; h->S = S; h->M = M; h->Sp = Sp; h->Mp = Mp; h->N64 = N64; h->Kcap = Kcap; h->k = k;
  h->max_picks = q.max_picks;
  h->mc = std::min(Mp, (budget - fixed) / (k * nrt * 8) / PC_NB * PC_NB);
  const int npc = (int)std::min<int64_t>(k, std::max<int64_t>(1, (budget - fixed) / (N64 * colsmax * 8)));
  // host staging of the small arrays
  std::vector<double> hom((size_t)Sp, 0.0), htau((size_t)k), hfl((size_t)k);
  if (q.w_ref) {
    double s = 0.0;
    for (int64_t i = 0; i < S; ++i) s += q.w_ref[i];
    for (int64_t i = 0; i < S; ++i) hom[(size_t)i] = q.w_ref[i] / s;
  } else {
    for (int64_t i = 0; i < S; ++i) hom[(size_t)i] = 1.0 / (double)S;
  }
  for (int64_t p = 0; p < k; ++p) {
    htau[(size_t)p] = q.tau ? q.tau[p] : m->h_noise[(size_t)p];
    hfl[(size_t)p] = q.min_variance * m->h_kdiag[(size_t)p];
  }
  DevScope sc(st);
  double *KT = nullptr;
  const int rc = [&]() -> int {
    GP_TRY(dev_alloc(&h->V1, k * Kcap * Sp));
    GP_TRY(dev_alloc(&h->V2, k * Kcap * Mp));
    GP_TRY(dev_alloc(&h->Xref, Sp * d));
    GP_TRY(dev_alloc(&h->Xcand, Mp * d));
    GP_TRY(dev_alloc(&h->omega, Sp));
    GP_TRY(dev_alloc(&h->pcw, k));
    GP_TRY(dev_alloc(&h->tau, k));
    GP_TRY(dev_alloc(&h->floorv, k));
    GP_TRY(dev_alloc(&h->dstar, k));
    GP_TRY(dev_alloc(&h->iv, k));
    GP_TRY(dev_alloc(&h->den, k * Mp));
    GP_TRY(dev_alloc(&h->cdiag, k * Sp));
    GP_TRY(dev_alloc(&h->part, k * nrt * h->mc));
    GP_TRY(dev_alloc(&h->score, Mp));
    GP_TRY(dev_alloc(&h->score_pc, k * Mp));
    GP_TRY(sc.alloc(&KT, (int64_t)npc * N64 * colsmax));
    GP_HIP(hipMemsetAsync(h->V1, 0, sizeof(double) * (size_t)(k * Kcap * Sp), st));
    GP_HIP(hipMemsetAsync(h->V2, 0, sizeof(double) * (size_t)(k * Kcap * Mp), st));
    GP_HIP(hipMemsetAsync(h->Xref, 0, sizeof(double) * (size_t)(Sp * d), st));
    GP_HIP(hipMemsetAsync(h->Xcand, 0, sizeof(double) * (size_t)(Mp * d), st));
    GP_TRY(gather_rows(ref, 0, S, h->Xref, st));
    GP_HIP(hipMemcpyAsync(h->Xcand, dXcand, sizeof(double) * (size_t)(M * d), hipMemcpyDeviceToDevice, st));
    GP_TRY(upload(h->omega, hom.data(), Sp, st));
    GP_TRY(upload(h->pcw, q.pc_weight, k, st));
    GP_TRY(upload(h->tau, htau.data(), k, st));
    GP_TRY(upload(h->floorv, hfl.data(), k, st));
    // V of both sets, PCs in chunks through the one KT array
    for (int set = 0; set < 2; ++set) {
      const int64_t cols = set ? Mp : Sp, n = set ? M : S;
      double *V = set ? h->V2 : h->V1;
      for (int p0 = 0; p0 < (int)k; p0 += npc) {
        const int np = std::min<int>(npc, (int)k - p0);
        KmatArgs g;
        g.A = m->Xtr; g.sa = m->dp; g.na = N; g.B = set ? h->Xcand : h->Xref; g.sb = d; g.nb = n; g.p0 = p0;
        g.out = KT; g.ldo = cols; g.strideo = N64 * cols; g.rows = N64; g.cols = cols;
        GP_TRY(launch_kmat(m, g, np, st));
        GP_TRY(launch_v(m, p0, np, KT, V + (int64_t)p0 * Kcap * cols, N64, cols, st, Kcap * cols));
      }
    }
    hipLaunchKernelGGL(design_den0_kernel, dim3((unsigned)((Sp + 255) / 256), (unsigned)k), dim3(256), 0, st, h->V1, Kcap,
                       Sp, N64, m->constv, (const double *)nullptr, h->cdiag);
    hipLaunchKernelGGL(design_den0_kernel, dim3((unsigned)((Mp + 255) / 256), (unsigned)k), dim3(256), 0, st, h->V2, Kcap,
                       Mp, N64, m->constv, (const double *)h->tau, h->den);
    hipLaunchKernelGGL(design_wsum_kernel, dim3((unsigned)k), dim3(256), 0, st, h->cdiag, Sp, Sp, h->omega, 0, h->iv);
    GP_HIP(hipGetLastError());
    GP_HIP(hipStreamSynchronize(st));   // the staging vectors and KT go
    return GPEMU_OK;
  }();
  if (rc != GPEMU_OK) {
    (void)hipStreamSynchronize(st);
    design_free(h);
    return rc;
  }
  *out = h;
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_design_create_dev(gpemu_design **out, gpemu_model *m, const double *dXref, int64_t n_blocks,
                            int64_t block_rows, int64_t block_stride_rows, const double *w_ref, int64_t M,
                            const double *dXcand, const double *pc_weight, const double *tau, double min_variance,
                            int64_t max_picks, int64_t workspace_bytes, void *stream) {
  GP_ARG(out && m && dXref && dXcand, "null pointer");
  *out = nullptr;
  const RowsView ref{dXref, n_blocks, block_rows, block_stride_rows * m->d, (int)m->d};
  GP_TRY(rows_check(ref));
  GP_ARG(n_blocks <= 4194240 / block_rows, "S = n_blocks * block_rows must be at most 4194240");
  DesignSpec q;
  q.S = n_blocks * block_rows; q.M = M; q.max_picks = max_picks; q.workspace_bytes = workspace_bytes;
  q.w_ref = w_ref; q.pc_weight = pc_weight; q.tau = tau; q.min_variance = min_variance;
  GP_TRY(design_check(m, q));
  GP_HIP(hipSetDevice(m->device));
  if (stream) GP_HIP(hipStreamSynchronize((hipStream_t)stream));
  return design_build(out, m, q, ref, dXcand);
}

int gpemu_design_create(gpemu_design **out, gpemu_model *m, int64_t S, const double *Xref, const double *w_ref,
                        int64_t M, const double *Xcand, const double *pc_weight, const double *tau,
                        double min_variance, int64_t max_picks, int64_t workspace_bytes) {
  GP_ARG(out && m && Xref && Xcand, "null pointer");
  *out = nullptr;
  DesignSpec q;
  q.S = S; q.M = M; q.max_picks = max_picks; q.workspace_bytes = workspace_bytes;
  q.w_ref = w_ref; q.pc_weight = pc_weight; q.tau = tau; q.min_variance = min_variance;
  GP_TRY(design_check(m, q));
  for (int64_t i = 0; i < S * m->d; ++i) GP_ARG(std::isfinite(Xref[i]), "Xref contains NaN or infinity");
  for (int64_t i = 0; i < M * m->d; ++i) GP_ARG(std::isfinite(Xcand[i]), "Xcand contains NaN or infinity");
  GP_HIP(hipSetDevice(m->device));
  int64_t budget = 0;
  GP_TRY(design_budget(m, q, &budget));   // (asked again by design_build: the copies below count against the free memory)
  hipStream_t st = m->stream;
  DevScope sc(st);
  double *dR = nullptr, *dC = nullptr;
  GP_TRY(sc.alloc(&dR, S * m->d));
  GP_TRY(sc.alloc(&dC, M * m->d));
  GP_TRY(upload(dR, Xref, S * m->d, st));
  GP_TRY(upload(dC, Xcand, M * m->d, st));
  const RowsView ref{dR, 1, S, S * m->d, (int)m->d};
  return design_build(out, m, q, ref, dC);
}

int gpemu_design_scores(gpemu_design *h, double *score, double *score_pc) {
  GP_ARG(h && score, "null pointer");
  gpemu_model *m = h->m;
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  design_path_count(GPEMU_DESIGN_PATH_SCORES);
  const int kind = kstar_kind(m);
  ScoreArgs g;
  g.V1 = h->V1; g.V2 = h->V2; g.Sp = h->Sp; g.Mp = h->Mp; g.Kcap = h->Kcap; g.N64 = h->N64;
  g.nk1 = (int)(round_up(m->N, 16) / 16); g.nk2 = (int)(round_up(h->n_picks, 16) / 16);
  g.Xref = h->Xref; g.Xcand = h->Xcand; g.omega = h->omega; g.S = h->S; g.M = h->M; g.ldp = h->mc; g.part = h->part;
  g.ls = m->ls; g.constv = m->constv; g.dp = m->dp; g.d = (int)m->d;
  if (kind == 4) g.mn = matern_nu_constants(m->nu);
  const int nrt = (int)(h->Sp / PC_NB);
  for (int64_t c0 = 0; c0 < h->Mp; c0 += h->mc) {
    const int64_t nc = std::min(h->mc, h->Mp - c0);
    g.c0 = c0;
    design_path_count(GPEMU_DESIGN_PATH_CHUNK);
    design_path_count(m->dp == DPAD ? GPEMU_DESIGN_PATH_DP8 : GPEMU_DESIGN_PATH_DP16);
    design_path_count(GPEMU_DESIGN_PATH_KIND_RBF + kind);
    const dim3 grid((unsigned)(nc / PC_NB), (unsigned)nrt, (unsigned)h->k);
    GP_TRY(with_kind_dp(m, [&](auto kd, auto dpv) {
      hipLaunchKernelGGL((design_score_kernel<decltype(kd)::value, decltype(dpv)::value>), grid, dim3(256), 0, st, g);
      return GPEMU_OK;
    }));
    GP_HIP(hipGetLastError());
    FinishArgs f;
    f.part = h->part; f.ldp = h->mc; f.nc = nc; f.c0 = c0; f.M = h->M; f.Mp = h->Mp; f.nrt = nrt; f.k = (int)h->k;
    f.den = h->den; f.pcw = h->pcw; f.floorv = h->floorv; f.score = h->score; f.score_pc = h->score_pc;
    hipLaunchKernelGGL(design_finish_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, f);
    GP_HIP(hipGetLastError());
  }
  GP_HIP(hipMemcpyAsync(score, h->score, sizeof(double) * (size_t)h->M, hipMemcpyDeviceToHost, st));
  if (score_pc)
    GP_HIP(hipMemcpy2DAsync(score_pc, sizeof(double) * (size_t)h->M, h->score_pc, sizeof(double) * (size_t)h->Mp,
                            sizeof(double) * (size_t)h->M, (size_t)h->k, hipMemcpyDeviceToHost, st));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_design_condition(gpemu_design *h, int64_t candidate) {
  GP_ARG(h, "null pointer");
  GP_ARG(candidate >= 0 && candidate < h->M, "candidate out of range");
  GP_ARG(h->n_picks < h->max_picks, "more picks than max_picks");
  gpemu_model *m = h->m;
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  design_path_count(GPEMU_DESIGN_PATH_COLUMN);
  hipLaunchKernelGGL(design_pick_kernel, dim3(1), dim3(64), 0, st, h->den, h->Mp, candidate, (int)h->k, h->dstar);
  GP_HIP(hipGetLastError());
  ColumnArgs g;
  g.V1 = h->V1; g.V2 = h->V2; g.Sp = h->Sp; g.Mp = h->Mp; g.Kcap = h->Kcap; g.N64 = h->N64; g.S = h->S; g.M = h->M;
  g.cstar = candidate; g.j = (int)h->n_picks; g.Xref = h->Xref; g.Xcand = h->Xcand; g.dstar = h->dstar;
  g.floorv = h->floorv; g.den = h->den; g.ls = m->ls; g.constv = m->constv; g.dp = m->dp; g.d = (int)m->d;
  if (kstar_kind(m) == 4) g.mn = matern_nu_constants(m->nu);
  const dim3 grid((unsigned)((h->Sp + h->Mp + 255) / 256), (unsigned)h->k);
  GP_TRY(with_kind_dp(m, [&](auto kd, auto dpv) {
    hipLaunchKernelGGL((design_column_kernel<decltype(kd)::value, decltype(dpv)::value>), grid, dim3(256), 0, st, g);
    return GPEMU_OK;
  }));
  GP_HIP(hipGetLastError());
  hipLaunchKernelGGL(design_wsum_kernel, dim3((unsigned)h->k), dim3(256), 0, st,
                     (const double *)(h->V1 + (h->N64 + h->n_picks) * h->Sp), h->Kcap * h->Sp, h->Sp, h->omega, 1, h->iv);
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(st));
  h->n_picks += 1;
  return GPEMU_OK;
}

int gpemu_design_state(gpemu_design *h, double *iv, double *den, int64_t *n_picks) {
  GP_ARG(h && iv, "null pointer");
  GP_HIP(hipSetDevice(h->m->device));
  hipStream_t st = h->m->stream;
  GP_HIP(hipMemcpyAsync(iv, h->iv, sizeof(double) * (size_t)h->k, hipMemcpyDeviceToHost, st));
  if (den)
    GP_HIP(hipMemcpy2DAsync(den, sizeof(double) * (size_t)h->M, h->den, sizeof(double) * (size_t)h->Mp,
                            sizeof(double) * (size_t)h->M, (size_t)h->k, hipMemcpyDeviceToHost, st));
  GP_HIP(hipStreamSynchronize(st));
  if (n_picks) *n_picks = h->n_picks;
  return GPEMU_OK;
}

int gpemu_design_destroy(gpemu_design *h) {
  if (!h) return GPEMU_OK;
  (void)hipSetDevice(h->m->device);
  (void)hipStreamSynchronize(h->m->stream);
  design_free(h);
  return GPEMU_OK;
}

int gpemu_design_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_DESIGN, out, n); }

}  // extern "C"
