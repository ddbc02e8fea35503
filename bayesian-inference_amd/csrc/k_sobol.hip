// Global (variance-based) sensitivity of the emulators: the pick-freeze PC means and their moments (gpemu_gp_mean_pick_freeze,
// gpemu_sobol_moments*).
//
// For base matrices A, B [n][d] the Sobol' estimators (Saltelli et al. 2010, Jansen 1999) need the GP means of the rows
// A_r, B_r and AB_i,r (A_r with coordinate i from B_r), i < d: d + 2 rows that differ from each other in one
// coordinate.  Only the MEANS are needed, so K_* is never stored and Wt never read.
//
// sobol_mean_kernel<KIND, DP>: one wave = 64 base rows of one PC p (grid: row tiles x PCs); it walks the training rows
// j in order.  x_j, alpha_pj and 1 / ls_p are the same for every lane: the loads are wave-uniform (the scalar cache
// serves them), the base rows' coordinates stay in registers.  Per (base row, j):
//     t^A_l = ((a_l - x_jl) / ls_pl)^2,  t^B_l likewise                            2 d squared scaled differences, once
//     r2_A = sum_l t^A_l,  r2_B = sum_l t^B_l                                       in index order
//     r2_i = (sum_{l < i} t^A_l + t^B_i) + sum_{l > i} t^A_l                        prefix and suffix sums of t^A
// O(d) operations for the d + 2 distances, and every sum is a sum of non-negative terms: no distance is formed by a
// cancellation, so the error of r2 is RELATIVE, (d + 6) u r2 -- the Matern-0.5 / nu < 1 hazard of the expanded form
// (predict_dev.h: kstar_direct_r2; exp(-r) is not flat at 0) does not arise, and a row AB_i that lands ON a training
// point gets r2 = 0 exactly.  A lane whose a_i == b_i (row AB_i IS row A) takes r2_A itself, so that B = A gives
// z(AB_i) == z(A) bit for bit.  Kernel values: exp_neg (predict_dev.h) with its table in LDS; kind 4 through the
// out-of-line matern_nu_value_call.  mean = sum_j alpha_j (k_j + const) in blocks of 16 training rows (inner sums in
// j order, the block sums added in block order): a fixed order that does not depend on the launch.
//
// Moments.  Rows belong to batch floor(r T / n); every batch is cut into slices of at most SB_SLICE rows (a rule of n
// and T only).  A chunk of the run is a set of whole consecutive slices whose means fit the workspace.  Per slice
//   sobol_matrix_kernel   C2 = sum (zA - c)(zA - c)^T + (zB - c)(zB - c)^T;  per i  M_i = sum (zB - c) D_i^T,
//                         D_i = sum D_i D_i^T with D_i = z(AB_i) - z(A): one thread per matrix entry, rows in blocks
//                         of 16 (inner sums in row order, block sums in block order);
//   sobol_vector_kernel   sum (zA - c), sum (zB - c), per i sum D_i, the same way;
// then sobol_combine_kernel adds the slices of a batch in slice order (blocks of 16 again).  No floating-point
// atomics; a partial sum covers a slice fixed by n and T, so the bits do not depend on the workspace or on the run.
// The pivot c is the mean of z over the first min(n, SB_PIVOT) rows of A and of B, computed first (its own pass of
// the mean kernel without the AB_i rows) and returned: the host re-centres about the true mean with a small correction.
//
// Second order (gpemu_sobol_moments_pairs).  The pair rows AB_ij (A_r with coordinates i < j from B_r) take
// slots of their own behind the d + 2, filled by sobol_pair_mean_kernel: grid z = one FIRST index i, whose partners j > i
// stay in registers (at most DP - 1 accumulators: no more than sobol_mean_kernel holds).  For fixed i the kernel walks j
// upward with a running sum,
//     r2_ij = ((sum_{l < i} t^A_l + t^B_i) + sum_{i < l < j} t^A_l + t^B_j) + sum_{l > j} t^A_l
// again a sum of non-negative terms, every term through at most d - 1 additions.  A lane with a_i == b_i has a row
// AB_ij that IS the row AB_j (with a_j == b_j: AB_i; with both: A), whose mean sobol_mean_kernel has already written to
// its slot of the same chunk: the lane stores THAT value.  Writing the same association in both kernels does not give
// the same bits (the compiler contracts the two kernels' sums into different fma chains: measured), a copy does,
// whatever the compiler: B = A gives exact zeros, a shared column D_ij = D_j.  sobol_pair_matrix_kernel /
// sobol_pair_vector_kernel are the siblings of
// the two slice kernels for M2_ij = sum (zB - c) D_ij^T, D2_ij = sum D_ij D_ij^T and sum D_ij; sobol_combine_kernel serves
// both.  The first-order kernels are untouched: the entry's first-order outputs are gpemu_sobol_moments' bytes.
#include <algorithm>

#include "internal.h"
#include "predict_dev.h"
#include "rows_dev.h"
#include "wg_dev.h"

namespace gpemu {

constexpr int SB_SLICE = 256;       // most rows per slice
constexpr int64_t SB_PIVOT = 1024;  // rows of A and of B behind the pivot
constexpr int SB_BLK = 16;          // summation block (training rows, base rows, slices)
constexpr int SB_MAXD = DPAD_WIDE, SB_MAXK = 64;

static inline void sobol_path_count(int path) { count_path(PATHS_SOBOL, path); }   // enum gpemu_sobol_path

// base kernel from the squared scaled distance (kinds 0 - 3: the closed forms on exp_neg; kind 4: matern_dev.h)
template <int KIND>
__device__ __forceinline__ double sobol_base(double r2, const double *tab, const MaternNu &mn) {
  if (KIND == 0) return exp_neg(-0.5 * r2, tab);
  const double r = sqrt(r2);
  if (KIND == 4) return matern_nu_value_call(mn, r);
  if (KIND == 1) return exp_neg(-r, tab);
  const double t = r * ((KIND == 2) ? 1.7320508075688772 : 2.23606797749979);
  const double e = exp_neg(-t, tab);
  if (KIND == 2) return (1.0 + t) * e;
  return (1.0 + t + t * t * (1.0 / 3.0)) * e;
}

struct SobolMeanArgs {
  const double *A = nullptr, *B = nullptr;   // [n][d] raw rows
  int64_t r0 = 0, nr = 0;                    // rows [r0, r0 + nr) of A and B
  double *Z = nullptr;                       // [d + 2][zs][k]: slot 0 A, 1 B, 2 + i AB_i; row r at index r - r0
  int64_t zs = 0;
  int64_t N = 0, Npad = 0;
  int d = 1, k = 1, has_const = 0, base_only = 0;
  MaternNu mn;
};

template <int KIND, int DP>
__global__ __launch_bounds__(64) void sobol_mean_kernel(SobolMeanArgs g, const double *__restrict__ Xtr,
                                                        const double *__restrict__ ls,
                                                        const double *__restrict__ alpha,
                                                        const double *__restrict__ constv) {
  __shared__ double s_tab[32];
  const int lane = threadIdx.x;
  if (lane < 32) s_tab[lane] = c_exp2_32[lane];
  __syncthreads();
  const int p = blockIdx.y;
  const int64_t rl = (int64_t)blockIdx.x * 64 + lane;
  const bool live = rl < g.nr;
  const int64_t r = g.r0 + (live ? rl : 0);
  const int d = g.d;
  double qa[DP], qb[DP], inv[DP];
#pragma unroll
  for (int l = 0; l < DP; ++l) {
    qa[l] = (l < d) ? g.A[r * d + l] : 0.0;
    qb[l] = (l < d) ? g.B[r * d + l] : 0.0;
    inv[l] = 1.0 / ls[(int64_t)p * DP + l];     // padded dimensions: ls = 1, coordinates 0
  }
  const double cst = g.has_const ? constv[p] : 0.0;
  const double *al = alpha + (int64_t)p * g.Npad;
  double accA = 0.0, accB = 0.0, acc[DP];
#pragma unroll
  for (int i = 0; i < DP; ++i) acc[i] = 0.0;

  for (int64_t j0 = 0; j0 < g.N; j0 += SB_BLK) {
    const int nj = (int)((g.N - j0 < SB_BLK) ? g.N - j0 : SB_BLK);
    double bA = 0.0, bB = 0.0, bs[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) bs[i] = 0.0;
    for (int jj = 0; jj < nj; ++jj) {
      const int64_t j = j0 + jj;
      const double *x = Xtr + j * DP;           // wave-uniform
      const double a_j = al[j];
      double ta[DP], tb[DP];
#pragma unroll
      for (int l = 0; l < DP; ++l) {
        const double xl = x[l];
        const double da = (qa[l] - xl) * inv[l];
        const double db = (qb[l] - xl) * inv[l];
        ta[l] = da * da;
        tb[l] = db * db;
      }
      // suffix sums of t^A: suf[i] = sum_{l > i} ta[l]; the prefix runs along with i below
      double suf[DP];
      suf[DP - 1] = 0.0;
#pragma unroll
      for (int l = DP - 2; l >= 0; --l) suf[l] = suf[l + 1] + ta[l + 1];
      double r2A = 0.0, r2B = 0.0;
#pragma unroll
      for (int l = 0; l < DP; ++l) {
        r2A += ta[l];
        r2B += tb[l];
      }
      bA = fma(a_j, sobol_base<KIND>(r2A, s_tab, g.mn) + cst, bA);
      bB = fma(a_j, sobol_base<KIND>(r2B, s_tab, g.mn) + cst, bB);
      if (!g.base_only) {
        double pre = 0.0;
#pragma unroll
        for (int i = 0; i < DP; ++i) {
          if (i < d) {                          // wave-uniform
            double r2 = (pre + tb[i]) + suf[i];
            r2 = (qa[i] == qb[i]) ? r2A : r2;   // the row AB_i is the row A
            bs[i] = fma(a_j, sobol_base<KIND>(r2, s_tab, g.mn) + cst, bs[i]);
          }
          pre += ta[i];
        }
      }
    }
    accA += bA;
    accB += bB;
#pragma unroll
    for (int i = 0; i < DP; ++i) acc[i] += bs[i];
  }
  if (!live) return;
  double *z = g.Z + rl * g.k + p;
  const int64_t slot = g.zs * g.k;
  z[0] = accA;
  z[slot] = accB;
  if (!g.base_only) {
#pragma unroll
    for (int i = 0; i < DP; ++i)
      if (i < d) z[(int64_t)(2 + i) * slot] = acc[i];
  }
}

// counted = false: a launch on behalf of gpemu_sobol_moments_pairs, which keeps counters of its own
static int launch_sobol_mean(const gpemu_model *m, SobolMeanArgs g, hipStream_t st, bool counted = true) {
  g.N = m->N; g.Npad = m->Npad; g.d = (int)m->d; g.k = (int)m->k; g.has_const = m->has_const;
  const int kind = kstar_kind(m);
  if (kind == 4) g.mn = matern_nu_constants(m->nu);
  if (counted) {
    sobol_path_count(m->dp == DPAD ? GPEMU_SOBOL_PATH_DP8 : GPEMU_SOBOL_PATH_DP16);
    sobol_path_count(GPEMU_SOBOL_PATH_KIND0 + kind);
  }
  dim3 grid((unsigned)((g.nr + 63) / 64), (unsigned)m->k), block(64);
  GP_TRY(with_base_kind(kind, [&](auto kd) {
    constexpr int K = decltype(kd)::value;
    if (m->dp == DPAD)
      hipLaunchKernelGGL((sobol_mean_kernel<K, DPAD>), grid, block, 0, st, g, m->Xtr, m->ls, m->alpha, m->constv);
    else
      hipLaunchKernelGGL((sobol_mean_kernel<K, DPAD_WIDE>), grid, block, 0, st, g, m->Xtr, m->ls, m->alpha, m->constv);
    return GPEMU_OK;
  }));
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

// ---- second order: the pair rows AB_ij ---------------------------------------------------------------------------------
struct SobolPairMeanArgs {
  const double *A = nullptr, *B = nullptr;   // [n][d] raw rows
  int64_t r0 = 0, nr = 0;                    // rows [r0, r0 + nr) of A and B
  double *Z = nullptr;                       // [n_pairs][zs][k]: the pair slots; row r at index r - r0
  const double *Z1 = nullptr;                // [d + 2][zs][k]: the first-order slots of the same rows, already written
  int64_t zs = 0;
  int64_t N = 0, Npad = 0;
  int d = 2, k = 1, has_const = 0;
  unsigned char first[SB_MAXD] = {};         // the first index of grid plane z
  short slot[SB_MAXD * SB_MAXD] = {};        // slot[i * SB_MAXD + j] = the pair's slot, -1: not asked for
  MaternNu mn;
};

// grid (row tiles, PCs, first indices): one wave = 64 base rows of one PC and one first index i = g.first[blockIdx.z]; the
// walk over l is unrolled and its three branches (l < i, l == i, l > i) are wave-uniform, so every register array keeps
// constant indices
template <int KIND, int DP>
__global__ __launch_bounds__(64) void sobol_pair_mean_kernel(SobolPairMeanArgs g, const double *__restrict__ Xtr,
                                                             const double *__restrict__ ls,
                                                             const double *__restrict__ alpha,
                                                             const double *__restrict__ constv) {
  __shared__ double s_tab[32];
  const int lane = threadIdx.x;
  if (lane < 32) s_tab[lane] = c_exp2_32[lane];
  __syncthreads();
  const int p = blockIdx.y;
  const int i = g.first[blockIdx.z];
  const int64_t rl = (int64_t)blockIdx.x * 64 + lane;
  const bool live = rl < g.nr;
  const int64_t r = g.r0 + (live ? rl : 0);
  const int d = g.d;
  double qa[DP], qb[DP], inv[DP];
  bool eq_i = false;
  unsigned want = 0;                            // bit l: the pair (i, l) was asked for (wave-uniform)
#pragma unroll
  for (int l = 0; l < DP; ++l) {
    qa[l] = (l < d) ? g.A[r * d + l] : 0.0;
    qb[l] = (l < d) ? g.B[r * d + l] : 0.0;
    inv[l] = 1.0 / ls[(int64_t)p * DP + l];     // padded dimensions: ls = 1, coordinates 0
    if (l == i) eq_i = qa[l] == qb[l];
    if (l > i && l < d && g.slot[i * SB_MAXD + l] >= 0) want |= 1u << l;
  }
  const double cst = g.has_const ? constv[p] : 0.0;
  const double *al = alpha + (int64_t)p * g.Npad;
  double acc[DP];
#pragma unroll
  for (int l = 0; l < DP; ++l) acc[l] = 0.0;

  for (int64_t j0 = 0; j0 < g.N; j0 += SB_BLK) {
    const int nj = (int)((g.N - j0 < SB_BLK) ? g.N - j0 : SB_BLK);
    double bs[DP];
#pragma unroll
    for (int l = 0; l < DP; ++l) bs[l] = 0.0;
    for (int jj = 0; jj < nj; ++jj) {
      const int64_t j = j0 + jj;
      const double *x = Xtr + j * DP;           // wave-uniform
      const double a_j = al[j];
      double ta[DP], tb[DP];
#pragma unroll
      for (int l = 0; l < DP; ++l) {
        const double xl = x[l];
        const double da = (qa[l] - xl) * inv[l];
        const double db = (qb[l] - xl) * inv[l];
        ta[l] = da * da;
        tb[l] = db * db;
      }
      double suf[DP];                           // suf[l] = sum_{m > l} ta[m]
      suf[DP - 1] = 0.0;
#pragma unroll
      for (int l = DP - 2; l >= 0; --l) suf[l] = suf[l + 1] + ta[l + 1];
      // pre: the prefix of t^A below i; run: (pre + t^B_i) + the t^A between i and l
      double pre = 0.0, run = 0.0;
#pragma unroll
      for (int l = 0; l < DP; ++l) {
        if (l < i) {
          pre += ta[l];
        } else if (l == i) {
          run = pre + tb[l];
        } else {
          if ((want >> l) & 1u) {
            const double r2 = (run + tb[l]) + suf[l];
            bs[l] = fma(a_j, sobol_base<KIND>(r2, s_tab, g.mn) + cst, bs[l]);
          }
          run += ta[l];
        }
      }
    }
#pragma unroll
    for (int l = 0; l < DP; ++l) acc[l] += bs[l];
  }
  if (!live) return;
  double *z = g.Z + rl * g.k + p;
  const double *z1 = g.Z1 + rl * g.k + p;
  const int64_t slot = g.zs * g.k;
#pragma unroll
  for (int l = 1; l < DP; ++l)
    if ((want >> l) & 1u) {
      const bool eq_l = qa[l] == qb[l];
      double v = acc[l];
      // the row AB_il is the row AB_l (a_i == b_i), AB_i (a_l == b_l) or A (both): that row's mean, from its slot
      if (eq_i || eq_l) v = z1[(int64_t)(eq_i ? (eq_l ? 0 : 2 + l) : 2 + i) * slot];
      z[(int64_t)g.slot[i * SB_MAXD + l] * slot] = v;
    }
}

static inline void sobol_pairs_path_count(int path) { count_path(PATHS_SOBOL_PAIRS, path); }   // enum gpemu_sobol_pairs_path

// g.first / g.slot / nz: filled by the caller (sobol_moments_run)
static int launch_sobol_pair_mean(const gpemu_model *m, SobolPairMeanArgs g, int nz, hipStream_t st) {
  g.N = m->N; g.Npad = m->Npad; g.d = (int)m->d; g.k = (int)m->k; g.has_const = m->has_const;
  const int kind = kstar_kind(m);
  if (kind == 4) g.mn = matern_nu_constants(m->nu);
  sobol_pairs_path_count(m->dp == DPAD ? GPEMU_SOBOL_PAIRS_PATH_DP8 : GPEMU_SOBOL_PAIRS_PATH_DP16);
  sobol_pairs_path_count(GPEMU_SOBOL_PAIRS_PATH_KIND0 + kind);
  dim3 grid((unsigned)((g.nr + 63) / 64), (unsigned)m->k, (unsigned)nz), block(64);
  GP_TRY(with_base_kind(kind, [&](auto kd) {
    constexpr int K = decltype(kd)::value;
    if (m->dp == DPAD)
      hipLaunchKernelGGL((sobol_pair_mean_kernel<K, DPAD>), grid, block, 0, st, g, m->Xtr, m->ls, m->alpha, m->constv);
    else
      hipLaunchKernelGGL((sobol_pair_mean_kernel<K, DPAD_WIDE>), grid, block, 0, st, g, m->Xtr, m->ls, m->alpha, m->constv);
    return GPEMU_OK;
  }));
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

// sum of f(0) .. f(n - 1) in blocks of SB_BLK: inner sums in index order, the block sums added in block order
template <class Fn>
__device__ __forceinline__ double sobol_blocked_sum(int64_t n, Fn &&f) {
  double acc = 0.0;
  for (int64_t i0 = 0; i0 < n; i0 += SB_BLK) {
    const int64_t e = (i0 + SB_BLK < n) ? i0 + SB_BLK : n;
    double b = 0.0;
    for (int64_t i = i0; i < e; ++i) b += f(i);
    acc += b;
  }
  return acc;
}

// pivot[p] = mean of z over the m rows of A and of B in Z [2][zs][k] (slots A, B); one workgroup per PC: thread t adds
// rows t, t + 256, .. in order, then tree A of wg_dev.h
__global__ __launch_bounds__(256) void sobol_pivot_kernel(const double *__restrict__ Z, int64_t zs, int64_t m, int k,
                                                          double *__restrict__ pivot) {
  __shared__ double s[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t r = tid; r < m; r += 256) acc += Z[r * k + p] + Z[(zs + r) * k + p];
  acc = wg_sum_a<256>(acc, s);
  if (tid == 0) pivot[p] = acc / (double)(2 * m);
}

// the partial sums of one slice: [C2 k^2][M d k^2][D d k^2][sumA k][sumB k][sumD d k]
static inline int64_t sobol_part_stride(int64_t d, int64_t k) { return (1 + 2 * d) * k * k + (2 + d) * k; }

struct SobolSliceArgs {
  const double *Z = nullptr;        // the chunk's means [d + 2][zs][k]
  int64_t zs = 0, row0 = 0;         // the chunk's first row
  const int64_t *start = nullptr;   // [nslices + 1] first row of every slice (device)
  int64_t s0 = 0;                   // the chunk's first slice
  const double *pivot = nullptr;    // [k]
  double *part = nullptr;           // [nslices][stride]
  int64_t stride = 0;
  int d = 1, k = 1;
};

// grid (slices of the chunk, 1 + 2 d matrices, ceil(k^2 / 256)): y = 0: C2; 1 + i: M_i; 1 + d + i: D_i
__global__ __launch_bounds__(256) void sobol_matrix_kernel(SobolSliceArgs g) {
  const int e = blockIdx.z * 256 + threadIdx.x;
  const int k = g.k, d = g.d;
  if (e >= k * k) return;
  const int p = e / k, q = e % k;
  const int64_t s = g.s0 + blockIdx.x;
  const int64_t b = g.start[s] - g.row0, len = g.start[s + 1] - g.start[s];
  const int mi = blockIdx.y;
  const double cp = g.pivot[p], cq = g.pivot[q];
  const int64_t slot = g.zs * k;
  const double *zA = g.Z + b * k, *zB = zA + slot;
  double v;
  if (mi == 0) {
    v = sobol_blocked_sum(len, [&](int64_t r) {
      const double ap = zA[r * k + p] - cp, aq = zA[r * k + q] - cq;
      const double bp = zB[r * k + p] - cp, bq = zB[r * k + q] - cq;
      return fma(ap, aq, bp * bq);
    });
  } else if (mi <= d) {
    const double *zi = zA + (int64_t)(1 + mi) * slot;
    v = sobol_blocked_sum(len, [&](int64_t r) { return (zB[r * k + p] - cp) * (zi[r * k + q] - zA[r * k + q]); });
  } else {
    const double *zi = zA + (int64_t)(1 + mi - d) * slot;
    v = sobol_blocked_sum(len, [&](int64_t r) { return (zi[r * k + p] - zA[r * k + p]) * (zi[r * k + q] - zA[r * k + q]); });
  }
  g.part[s * g.stride + (int64_t)mi * k * k + e] = v;
}

// grid (slices of the chunk, 2 + d vectors): y = 0: sum (zA - c); 1: sum (zB - c); 2 + i: sum D_i
__global__ __launch_bounds__(64) void sobol_vector_kernel(SobolSliceArgs g) {
  const int p = threadIdx.x, k = g.k, d = g.d;
  if (p >= k) return;
  const int64_t s = g.s0 + blockIdx.x;
  const int64_t b = g.start[s] - g.row0, len = g.start[s + 1] - g.start[s];
  const int vi = blockIdx.y;
  const double cp = g.pivot[p];
  const int64_t slot = g.zs * k;
  const double *zA = g.Z + b * k;
  double v;
  if (vi < 2) {
    const double *z = zA + (int64_t)vi * slot;
    v = sobol_blocked_sum(len, [&](int64_t r) { return z[r * k + p] - cp; });
  } else {
    const double *zi = zA + (int64_t)vi * slot;
    v = sobol_blocked_sum(len, [&](int64_t r) { return zi[r * k + p] - zA[r * k + p]; });
  }
  g.part[s * g.stride + (int64_t)(1 + 2 * d) * k * k + (int64_t)vi * k + p] = v;
}

// the pair partial sums of one slice: [M2 P k^2][D2 P k^2][sumD2 P k]
static inline int64_t sobol_pair_part_stride(int64_t P, int64_t k) { return P * (2 * k * k + k); }

struct SobolPairSliceArgs {
  const double *Z = nullptr;        // the chunk's means [d + 2 + P][zs][k]
  int64_t zs = 0, row0 = 0;         // the chunk's first row
  const int64_t *start = nullptr;   // [nslices + 1] first row of every slice (device)
  int64_t s0 = 0;                   // the first slice of this launch
  const double *pivot = nullptr;    // [k]
  double *part = nullptr;           // [nslices][stride]
  int64_t stride = 0;
  int d = 2, k = 1, np = 1;
};

// grid (slices, 2 P matrices, ceil(k^2 / 256)): y < P: M2 of pair y; P + y: D2 of pair y; the sums of sobol_matrix_kernel
__global__ __launch_bounds__(256) void sobol_pair_matrix_kernel(SobolPairSliceArgs g) {
  const int e = blockIdx.z * 256 + threadIdx.x;
  const int k = g.k;
  if (e >= k * k) return;
  const int p = e / k, q = e % k;
  const int64_t s = g.s0 + blockIdx.x;
  const int64_t b = g.start[s] - g.row0, len = g.start[s + 1] - g.start[s];
  const int mi = blockIdx.y, pi = (mi < g.np) ? mi : mi - g.np;
  const int64_t slot = g.zs * k;
  const double *zA = g.Z + b * k, *zB = zA + slot, *zi = zA + (int64_t)(g.d + 2 + pi) * slot;
  double v;
  if (mi < g.np) {
    const double cp = g.pivot[p];
    v = sobol_blocked_sum(len, [&](int64_t r) { return (zB[r * k + p] - cp) * (zi[r * k + q] - zA[r * k + q]); });
  } else {
    v = sobol_blocked_sum(len, [&](int64_t r) { return (zi[r * k + p] - zA[r * k + p]) * (zi[r * k + q] - zA[r * k + q]); });
  }
  g.part[s * g.stride + (int64_t)mi * k * k + e] = v;
}

// grid (slices, P): sum D_ij of pair y
__global__ __launch_bounds__(64) void sobol_pair_vector_kernel(SobolPairSliceArgs g) {
  const int p = threadIdx.x, k = g.k;
  if (p >= k) return;
  const int64_t s = g.s0 + blockIdx.x;
  const int64_t b = g.start[s] - g.row0, len = g.start[s + 1] - g.start[s];
  const int pi = blockIdx.y;
  const double *zA = g.Z + b * k, *zi = zA + (int64_t)(g.d + 2 + pi) * g.zs * k;
  const double v = sobol_blocked_sum(len, [&](int64_t r) { return zi[r * k + p] - zA[r * k + p]; });
  g.part[s * g.stride + (int64_t)2 * g.np * k * k + (int64_t)pi * k + p] = v;
}

// out[t][e] = the sum over the slices [first[t], first[t + 1]) of part[.][e], e < stride; grid (ceil(stride / 256), T)
__global__ __launch_bounds__(256) void sobol_combine_kernel(const double *__restrict__ part, int64_t stride,
                                                            const int64_t *__restrict__ first,
                                                            double *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= stride) return;
  const int64_t t = blockIdx.y, s0 = first[t], ns = first[t + 1] - s0;
  out[t * stride + e] = sobol_blocked_sum(ns, [&](int64_t s) { return part[(s0 + s) * stride + e]; });
}

// the slices of n rows in T batches: batch t = rows [ceil(t n / T), ceil((t + 1) n / T)) cut into ceil(len / SB_SLICE)
// slices of nearly equal length.  start [nslices + 1], first [T + 1] (the first slice of every batch)
static void sobol_slices(int64_t n, int64_t T, std::vector<int64_t> &start, std::vector<int64_t> &first) {
  start.clear();
  first.clear();
  for (int64_t t = 0; t < T; ++t) {
    const int64_t b0 = (int64_t)(((__int128)t * n + T - 1) / T), b1 = (int64_t)(((__int128)(t + 1) * n + T - 1) / T);
    const int64_t len = b1 - b0, ns = (len + SB_SLICE - 1) / SB_SLICE;
    first.push_back((int64_t)start.size());
    for (int64_t s = 0; s < ns; ++s) start.push_back(b0 + s * len / ns);
  }
  first.push_back((int64_t)start.size());
  start.push_back(n);
}

static int sobol_check_model(const gpemu_model *m) {
  GP_ARG(m->d >= 1 && m->d <= SB_MAXD, "the model's d must be in 1 .. 16");
  GP_ARG(m->k >= 1 && m->k <= SB_MAXK, "the model's k must be in 1 .. 64");
  return GPEMU_OK;
}

static bool sobol_all_finite(const double *x, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) return false;
  return true;
}

struct SobolOut { double *pivot; int64_t *count; double *sumA, *sumB, *C2, *sumD, *M, *D; };   // host arrays
struct SobolPairOut {                 // the second-order part of a call: the pairs and their host arrays
  int64_t np = 0;
  const int32_t *pairs = nullptr;     // [np][2], checked by the caller
  double *sumD2 = nullptr, *M2 = nullptr, *D2 = nullptr;
};

// the body of gpemu_sobol_moments_dev (po == nullptr: its launches, allocations and counters exactly) and of
// gpemu_sobol_moments_pairs (po: the pair slots behind the d + 2 of every chunk, their slice sums beside the first-order
// ones, the counters of enum gpemu_sobol_pairs_path in place of enum gpemu_sobol_path's)
static int sobol_moments_run(gpemu_model *m, int64_t n, const double *dA, const double *dB, int64_t T,
                             int64_t workspace_bytes, const SobolOut &o, const SobolPairOut *po, hipStream_t st) {
  const int64_t d = m->d, k = m->k, P = po ? po->np : 0;
  const int64_t stride = sobol_part_stride(d, k), stride2 = sobol_pair_part_stride(P, k);
  const int64_t row_bytes = (d + 2 + P) * k * 8;
  const char *who = po ? "sobol_moments_pairs" : "sobol_moments";

  std::vector<int64_t> start, first;
  sobol_slices(n, T, start, first);
  const int64_t nslices = (int64_t)start.size() - 1;
  for (int64_t t = 0; t < T; ++t) o.count[t] = start[(size_t)first[(size_t)t + 1]] - start[(size_t)first[(size_t)t]];

  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t npiv = std::min(n, SB_PIVOT);
  int64_t cap = std::min(budget / row_bytes, n);          // rows of means the workspace holds
  if (cap < std::min<int64_t>(n, SB_SLICE)) {
    set_error("%s: out of memory: one slice of %lld rows needs %lld bytes of PC means; %lld bytes %s", who,
              (long long)std::min<int64_t>(n, SB_SLICE), (long long)(std::min<int64_t>(n, SB_SLICE) * row_bytes),
              (long long)budget, workspace_budget_name(workspace_bytes));
    return GPEMU_ERR_HIP;
  }

  // the pair kernel's tables: the first indices that occur (one grid plane each) and every pair's slot
  SobolPairMeanArgs pg;
  int nz = 0;
  if (po) {
    for (int e = 0; e < SB_MAXD * SB_MAXD; ++e) pg.slot[e] = -1;
    bool seen[SB_MAXD] = {};
    for (int64_t q = 0; q < P; ++q) {
      const int i = po->pairs[2 * q], j = po->pairs[2 * q + 1];
      pg.slot[i * SB_MAXD + j] = (short)q;
      seen[i] = true;
    }
    for (int i = 0; i < SB_MAXD; ++i)
      if (seen[i]) pg.first[nz++] = (unsigned char)i;
  }

  DevScope sc(st);
  double *Z = nullptr, *part = nullptr, *dpivot = nullptr, *dout = nullptr, *part2 = nullptr, *dout2 = nullptr;
  int64_t *dstart = nullptr, *dfirst = nullptr;
  GP_TRY(sc.alloc(&Z, std::max(cap * (d + 2 + P), 2 * npiv) * k));
  GP_TRY(sc.alloc(&part, nslices * stride));
  GP_TRY(sc.alloc(&dpivot, k));
  GP_TRY(sc.alloc(&dout, T * stride));
  GP_TRY(sc.alloc(&dstart, nslices + 1));
  GP_TRY(sc.alloc(&dfirst, T + 1));
  if (po) {
    GP_TRY(sc.alloc(&part2, nslices * stride2));
    GP_TRY(sc.alloc(&dout2, T * stride2));
  }
  GP_TRY(upload(dstart, start.data(), nslices + 1, st));
  GP_TRY(upload(dfirst, first.data(), T + 1, st));

  const bool own = !po;                                    // count in enum gpemu_sobol_path
  auto count_call = [&](int path) { own ? sobol_path_count(path) : sobol_pairs_path_count(path); };   // same order
  static_assert((int)GPEMU_SOBOL_PAIRS_PATH_CALL == (int)GPEMU_SOBOL_PATH_CALL &&
                (int)GPEMU_SOBOL_PAIRS_PATH_CHUNK == (int)GPEMU_SOBOL_PATH_CHUNK &&
                (int)GPEMU_SOBOL_PAIRS_PATH_WHOLE == (int)GPEMU_SOBOL_PATH_WHOLE, "the two enums share their head");
  count_call(GPEMU_SOBOL_PATH_CALL);
  // the pivot: the means of the first npiv rows of A and B
  SobolMeanArgs g;
  g.A = dA; g.B = dB; g.r0 = 0; g.nr = npiv; g.Z = Z; g.zs = npiv; g.base_only = 1;
  GP_TRY(launch_sobol_mean(m, g, st, own));
  hipLaunchKernelGGL(sobol_pivot_kernel, dim3((unsigned)k), dim3(256), 0, st, Z, npiv, npiv, (int)k, dpivot);
  GP_HIP(hipGetLastError());

  int64_t nchunks = 0;
  for (int64_t s0 = 0; s0 < nslices;) {
    int64_t s1 = s0 + 1;                                   // whole slices while their rows fit
    while (s1 < nslices && start[(size_t)s1 + 1] - start[(size_t)s0] <= cap) ++s1;
    const int64_t row0 = start[(size_t)s0], nr = start[(size_t)s1] - row0;
    count_call(GPEMU_SOBOL_PATH_CHUNK);
    ++nchunks;
    g = SobolMeanArgs();
    g.A = dA; g.B = dB; g.r0 = row0; g.nr = nr; g.Z = Z; g.zs = nr;
    GP_TRY(launch_sobol_mean(m, g, st, own));
    SobolSliceArgs a;
    a.Z = Z; a.zs = nr; a.row0 = row0; a.start = dstart; a.s0 = s0; a.pivot = dpivot; a.part = part; a.stride = stride;
    a.d = (int)d; a.k = (int)k;
    SobolPairSliceArgs a2;
    if (po) {
      pg.A = dA; pg.B = dB; pg.r0 = row0; pg.nr = nr; pg.Z = Z + (d + 2) * nr * k; pg.Z1 = Z; pg.zs = nr;
      GP_TRY(launch_sobol_pair_mean(m, pg, nz, st));
      a2.Z = Z; a2.zs = nr; a2.row0 = row0; a2.start = dstart; a2.pivot = dpivot; a2.part = part2; a2.stride = stride2;
      a2.d = (int)d; a2.k = (int)k; a2.np = (int)P;
    }
    for (int64_t c0 = s0; c0 < s1; c0 += 32768) {          // grid.x
      const int64_t nc = std::min<int64_t>(32768, s1 - c0);
      a.s0 = c0;
      hipLaunchKernelGGL(sobol_matrix_kernel, dim3((unsigned)nc, (unsigned)(1 + 2 * d), (unsigned)((k * k + 255) / 256)),
                         dim3(256), 0, st, a);
      GP_HIP(hipGetLastError());
      hipLaunchKernelGGL(sobol_vector_kernel, dim3((unsigned)nc, (unsigned)(2 + d)), dim3(64), 0, st, a);
      GP_HIP(hipGetLastError());
      if (po) {
        a2.s0 = c0;
        hipLaunchKernelGGL(sobol_pair_matrix_kernel, dim3((unsigned)nc, (unsigned)(2 * P), (unsigned)((k * k + 255) / 256)),
                           dim3(256), 0, st, a2);
        GP_HIP(hipGetLastError());
        hipLaunchKernelGGL(sobol_pair_vector_kernel, dim3((unsigned)nc, (unsigned)P), dim3(64), 0, st, a2);
        GP_HIP(hipGetLastError());
      }
    }
    s0 = s1;
  }
  if (nchunks == 1) count_call(GPEMU_SOBOL_PATH_WHOLE);
  for (int64_t t0 = 0; t0 < T; t0 += 32768) {              // grid.y
    const int64_t nt = std::min<int64_t>(32768, T - t0);
    hipLaunchKernelGGL(sobol_combine_kernel, dim3((unsigned)((stride + 255) / 256), (unsigned)nt), dim3(256), 0, st, part,
                       stride, dfirst + t0, dout + t0 * stride);
    GP_HIP(hipGetLastError());
    if (po) {
      hipLaunchKernelGGL(sobol_combine_kernel, dim3((unsigned)((stride2 + 255) / 256), (unsigned)nt), dim3(256), 0, st,
                         part2, stride2, dfirst + t0, dout2 + t0 * stride2);
      GP_HIP(hipGetLastError());
    }
  }

  std::vector<double> host((size_t)(T * stride)), host2((size_t)(T * stride2));
  GP_TRY(sc.download(host.data(), dout, T * stride));
  if (po) GP_TRY(sc.download(host2.data(), dout2, T * stride2));
  GP_TRY(sc.download(o.pivot, dpivot, k));
  GP_HIP(hipStreamSynchronize(st));
  const int64_t kk = k * k;
  for (int64_t t = 0; t < T; ++t) {
    const double *h = host.data() + t * stride;
    std::copy(h, h + kk, o.C2 + t * kk);
    std::copy(h + kk, h + (1 + d) * kk, o.M + t * d * kk);
    std::copy(h + (1 + d) * kk, h + (1 + 2 * d) * kk, o.D + t * d * kk);
    const double *v = h + (1 + 2 * d) * kk;
    std::copy(v, v + k, o.sumA + t * k);
    std::copy(v + k, v + 2 * k, o.sumB + t * k);
    std::copy(v + 2 * k, v + (2 + d) * k, o.sumD + t * d * k);
    if (po) {
      const double *h2 = host2.data() + t * stride2;
      std::copy(h2, h2 + P * kk, po->M2 + t * P * kk);
      std::copy(h2 + P * kk, h2 + 2 * P * kk, po->D2 + t * P * kk);
      std::copy(h2 + 2 * P * kk, h2 + 2 * P * kk + P * k, po->sumD2 + t * P * k);
    }
  }
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_sobol_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_SOBOL, out, n); }

int gpemu_gp_mean_pick_freeze(gpemu_model *m, int64_t n, const double *A, const double *B, double *Z_out) {
  GP_ARG(m && A && B && Z_out, "null pointer");
  GP_ARG(n >= 1, "n must be >= 1");
  GP_TRY(sobol_check_model(m));
  const int64_t d = m->d, k = m->k;
  GP_ARG(sobol_all_finite(A, n * d) && sobol_all_finite(B, n * d), "A or B contains NaN or infinity");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  DevScope sc(st);
  double *dA = nullptr, *dB = nullptr, *dZ = nullptr;
  GP_TRY(sc.alloc(&dA, n * d));
  GP_TRY(sc.alloc(&dB, n * d));
  GP_TRY(sc.alloc(&dZ, (d + 2) * n * k));
  GP_TRY(upload(dA, A, n * d, st));
  GP_TRY(upload(dB, B, n * d, st));
  SobolMeanArgs g;
  g.A = dA; g.B = dB; g.r0 = 0; g.nr = n; g.Z = dZ; g.zs = n;
  GP_TRY(launch_sobol_mean(m, g, st));
  GP_TRY(sc.download(Z_out, dZ, (d + 2) * n * k));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_sobol_moments_dev(gpemu_model *m, int64_t n, const double *dA, const double *dB, int64_t n_batches,
                            int64_t workspace_bytes, double *pivot, int64_t *count, double *sumA, double *sumB,
                            double *C2, double *sumD, double *M, double *D, void *stream) {
  GP_ARG(m && dA && dB, "null pointer");
  GP_ARG(pivot && count && sumA && sumB && C2 && sumD && M && D, "null output pointer");
  GP_ARG(n >= 1, "n must be >= 1");
  GP_ARG(n_batches >= 1 && n_batches <= n, "n_batches must be in 1 .. n");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_TRY(sobol_check_model(m));
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  SobolOut o{pivot, count, sumA, sumB, C2, sumD, M, D};
  return sobol_moments_run(m, n, dA, dB, n_batches, workspace_bytes, o, nullptr, st);
}

int gpemu_sobol_moments(gpemu_model *m, int64_t n, const double *A, const double *B, int64_t n_batches,
                        int64_t workspace_bytes, double *pivot, int64_t *count, double *sumA, double *sumB, double *C2,
                        double *sumD, double *M, double *D) {
  GP_ARG(m && A && B, "null pointer");
  GP_ARG(n >= 1, "n must be >= 1");
  GP_ARG(n_batches >= 1 && n_batches <= n, "n_batches must be in 1 .. n");
  GP_TRY(sobol_check_model(m));
  const int64_t d = m->d;
  GP_ARG(sobol_all_finite(A, n * d) && sobol_all_finite(B, n * d), "A or B contains NaN or infinity");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  DevScope sc(st);
  double *dA = nullptr, *dB = nullptr;
  GP_TRY(sc.alloc(&dA, n * d));
  GP_TRY(sc.alloc(&dB, n * d));
  GP_TRY(upload(dA, A, n * d, st));
  GP_TRY(upload(dB, B, n * d, st));
  return gpemu_sobol_moments_dev(m, n, dA, dB, n_batches, workspace_bytes, pivot, count, sumA, sumB, C2, sumD, M, D, st);
}

int gpemu_sobol_pairs_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_SOBOL_PAIRS, out, n); }

int gpemu_sobol_moments_pairs(gpemu_model *m, int64_t n, const double *A, const double *B, int64_t n_batches,
                              int64_t n_pairs, const int32_t *pairs, int64_t workspace_bytes, double *pivot,
                              int64_t *count, double *sumA, double *sumB, double *C2, double *sumD, double *M, double *D,
                              double *sumD2, double *M2, double *D2) {
  GP_ARG(m && A && B && pairs, "null pointer");
  GP_ARG(pivot && count && sumA && sumB && C2 && sumD && M && D && sumD2 && M2 && D2, "null output pointer");
  GP_ARG(n >= 1, "n must be >= 1");
  GP_ARG(n_batches >= 1 && n_batches <= n, "n_batches must be in 1 .. n");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_TRY(sobol_check_model(m));
  const int64_t d = m->d;
  GP_ARG(d >= 2, "a pair needs a model of d >= 2 parameters");
  GP_ARG(n_pairs >= 1 && n_pairs <= d * (d - 1) / 2, "n_pairs must be in 1 .. d (d - 1) / 2");
  bool asked[SB_MAXD * SB_MAXD] = {};
  for (int64_t q = 0; q < n_pairs; ++q) {
    const int64_t i = pairs[2 * q], j = pairs[2 * q + 1];
    GP_ARG(i >= 0 && j >= 0 && i < d && j < d, "a pair's index is outside 0 .. d - 1");
    GP_ARG(i < j, "a pair must be given as i < j");
    GP_ARG(!asked[i * SB_MAXD + j], "a pair is repeated");
    asked[i * SB_MAXD + j] = true;
  }
  GP_ARG(sobol_all_finite(A, n * d) && sobol_all_finite(B, n * d), "A or B contains NaN or infinity");
  GP_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  DevScope sc(st);
  double *dA = nullptr, *dB = nullptr;
  GP_TRY(sc.alloc(&dA, n * d));
  GP_TRY(sc.alloc(&dB, n * d));
  GP_TRY(upload(dA, A, n * d, st));
  GP_TRY(upload(dB, B, n * d, st));
  SobolOut o{pivot, count, sumA, sumB, C2, sumD, M, D};
  SobolPairOut po;
  po.np = n_pairs; po.pairs = pairs; po.sumD2 = sumD2; po.M2 = M2; po.D2 = D2;
  return sobol_moments_run(m, n, dA, dB, n_batches, workspace_bytes, o, &po, st);
}

}  // extern "C"
