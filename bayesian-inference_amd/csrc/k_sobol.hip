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

static int launch_sobol_mean(const gpemu_model *m, SobolMeanArgs g, hipStream_t st) {
  g.N = m->N; g.Npad = m->Npad; g.d = (int)m->d; g.k = (int)m->k; g.has_const = m->has_const;
  const int kind = kstar_kind(m);
  if (kind == 4) g.mn = matern_nu_constants(m->nu);
  sobol_path_count(m->dp == DPAD ? GPEMU_SOBOL_PATH_DP8 : GPEMU_SOBOL_PATH_DP16);
  sobol_path_count(GPEMU_SOBOL_PATH_KIND0 + kind);
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
  const int64_t d = m->d, k = m->k, T = n_batches;
  const int64_t stride = sobol_part_stride(d, k), row_bytes = (d + 2) * k * 8;

  std::vector<int64_t> start, first;
  sobol_slices(n, T, start, first);
  const int64_t nslices = (int64_t)start.size() - 1;
  for (int64_t t = 0; t < T; ++t) count[t] = start[(size_t)first[(size_t)t + 1]] - start[(size_t)first[(size_t)t]];

  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t npiv = std::min(n, SB_PIVOT);
  int64_t cap = std::min(budget / row_bytes, n);          // rows of means the workspace holds
  if (cap < std::min<int64_t>(n, SB_SLICE)) {
    set_error("sobol_moments: out of memory: one slice of %lld rows needs %lld bytes of PC means; %lld bytes %s",
              (long long)std::min<int64_t>(n, SB_SLICE), (long long)(std::min<int64_t>(n, SB_SLICE) * row_bytes),
              (long long)budget, workspace_budget_name(workspace_bytes));
    return GPEMU_ERR_HIP;
  }

  DevScope sc(st);
  double *Z = nullptr, *part = nullptr, *dpivot = nullptr, *dout = nullptr;
  int64_t *dstart = nullptr, *dfirst = nullptr;
  GP_TRY(sc.alloc(&Z, std::max(cap * (d + 2), 2 * npiv) * k));
  GP_TRY(sc.alloc(&part, nslices * stride));
  GP_TRY(sc.alloc(&dpivot, k));
  GP_TRY(sc.alloc(&dout, T * stride));
  GP_TRY(sc.alloc(&dstart, nslices + 1));
  GP_TRY(sc.alloc(&dfirst, T + 1));
  GP_TRY(upload(dstart, start.data(), nslices + 1, st));
  GP_TRY(upload(dfirst, first.data(), T + 1, st));

  sobol_path_count(GPEMU_SOBOL_PATH_CALL);
  // the pivot: the means of the first npiv rows of A and B
  SobolMeanArgs g;
  g.A = dA; g.B = dB; g.r0 = 0; g.nr = npiv; g.Z = Z; g.zs = npiv; g.base_only = 1;
  GP_TRY(launch_sobol_mean(m, g, st));
  hipLaunchKernelGGL(sobol_pivot_kernel, dim3((unsigned)k), dim3(256), 0, st, Z, npiv, npiv, (int)k, dpivot);
  GP_HIP(hipGetLastError());

  int64_t nchunks = 0;
  for (int64_t s0 = 0; s0 < nslices;) {
    int64_t s1 = s0 + 1;                                   // whole slices while their rows fit
    while (s1 < nslices && start[(size_t)s1 + 1] - start[(size_t)s0] <= cap) ++s1;
    const int64_t row0 = start[(size_t)s0], nr = start[(size_t)s1] - row0;
    sobol_path_count(GPEMU_SOBOL_PATH_CHUNK);
    ++nchunks;
    g = SobolMeanArgs();
    g.A = dA; g.B = dB; g.r0 = row0; g.nr = nr; g.Z = Z; g.zs = nr;
    GP_TRY(launch_sobol_mean(m, g, st));
    SobolSliceArgs a;
    a.Z = Z; a.zs = nr; a.row0 = row0; a.start = dstart; a.s0 = s0; a.pivot = dpivot; a.part = part; a.stride = stride;
    a.d = (int)d; a.k = (int)k;
    for (int64_t c0 = s0; c0 < s1; c0 += 32768) {          // grid.x
      const int64_t nc = std::min<int64_t>(32768, s1 - c0);
      a.s0 = c0;
      hipLaunchKernelGGL(sobol_matrix_kernel, dim3((unsigned)nc, (unsigned)(1 + 2 * d), (unsigned)((k * k + 255) / 256)),
                         dim3(256), 0, st, a);
      GP_HIP(hipGetLastError());
      hipLaunchKernelGGL(sobol_vector_kernel, dim3((unsigned)nc, (unsigned)(2 + d)), dim3(64), 0, st, a);
      GP_HIP(hipGetLastError());
    }
    s0 = s1;
  }
  if (nchunks == 1) sobol_path_count(GPEMU_SOBOL_PATH_WHOLE);
  for (int64_t t0 = 0; t0 < T; t0 += 32768) {              // grid.y
    const int64_t nt = std::min<int64_t>(32768, T - t0);
    hipLaunchKernelGGL(sobol_combine_kernel, dim3((unsigned)((stride + 255) / 256), (unsigned)nt), dim3(256), 0, st, part,
                       stride, dfirst + t0, dout + t0 * stride);
    GP_HIP(hipGetLastError());
  }

  std::vector<double> host((size_t)(T * stride));
  GP_TRY(sc.download(host.data(), dout, T * stride));
  GP_TRY(sc.download(pivot, dpivot, k));
  GP_HIP(hipStreamSynchronize(st));
  const int64_t kk = k * k;
  for (int64_t t = 0; t < T; ++t) {
    const double *h = host.data() + t * stride;
    std::copy(h, h + kk, C2 + t * kk);
    std::copy(h + kk, h + (1 + d) * kk, M + t * d * kk);
    std::copy(h + (1 + d) * kk, h + (1 + 2 * d) * kk, D + t * d * kk);
    const double *v = h + (1 + 2 * d) * kk;
    std::copy(v, v + k, sumA + t * k);
    std::copy(v + k, v + 2 * k, sumB + t * k);
    std::copy(v + 2 * k, v + (2 + d) * k, sumD + t * d * k);
  }
  return GPEMU_OK;
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

}  // extern "C"
