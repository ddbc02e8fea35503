// 2-D Gaussian kernel densities of parameter pairs (gpemu_kde2d*, gpemu_pair_moments_dev): the smooth
// off-diagonal panels of a corner plot from every sample, where the chain lies.
//
// A product Gaussian kernel factorises, so the density of pair (i, j) on a G x G product grid is a matrix product over
// the samples: Z = A B^T / (S 2 pi h_a h_b), A[a][s] = exp(-((g_a[a] - x_s) / h_a)^2 / 2), B[b][s] = the same of
// g_b, h_b and v_s = x_sj - beta x_si.  With beta = C_ij / C_ii the sheared coordinates (x, v) are uncorrelated in the
// sample, and the product kernel in them is the full-covariance kernel of scipy.stats.gaussian_kde at the points
// (g_a[a], g_b[b] + beta g_a[a]); beta = 0 is the axis-aligned product kernel.
//
// kde2d_partial_kernel<T>: workgroup (chunk of K2_CHUNK samples, T x T tile of the panel, pair), 256 threads = 4 waves
// (2 x 2, a T/2 x T/2 quarter of the tile each) -- the schedule of design_score_kernel.  T = 128 unless the whole panel
// fits 64 x 64: a generated operand value then feeds 128 multiply-adds, and a panel of G = 100 is one tile.  The samples
// of the chunk are staged K2_STAGE at a time (x, v and the rounding error of v, read through the RowsView); per k-tile
// of 16 samples every thread generates T / 16 values of A and as many of B into LDS ([k][T + 16] doubles: the 16 lanes
// of one k read 16 consecutive doubles, the two k of a 32-lane half lie T + 16 doubles = 16 mod 32 apart -- no bank
// conflict for the 8-byte reads), and every wave runs 4 (T / 32)^2 v_mfma_f64_16x16x4_f64 on it: one exp per T / 2
// multiply-adds.  Rows of the tile beyond G and samples beyond the chunk generate 0; only the G x G part is stored.
// kde2d_sum_kernel: one thread per element adds its partial tiles in chunk order and scales once.  No floating-point
// atomics: the order of every sum is fixed by S and G.
//
// pm_*: the pooled mean, the full covariance (divisor S) and the extents of fma(-beta, x_i, x_j) of rows in blocks, as
// tree A (wg_dev.h) over MOM_ROWS rows per workgroup like moments_partial_kernel; the blocks' partials of the sums go
// through the same final stage (launch_moments_final).
#include <algorithm>
#include <cmath>
#include <vector>

#include "internal.h"
#include "rows_dev.h"
#include "wg_dev.h"

namespace gpemu {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int K2_T_SMALL = 64;      // the tile of the panel a workgroup owns where the panel fits it (G <= 64) ...
constexpr int K2_T = 128;           // ... and otherwise
constexpr int K2_GK = 16;           // samples per k-tile
constexpr int K2_SKPAD = 16;        // padding of an operand k-row in LDS: rows lie 16 mod 32 doubles apart
constexpr int K2_STAGE = 256;       // samples staged at a time: one per thread
constexpr int K2_CHUNK = 8192;      // samples per partial tile
constexpr int K2_MAX_D = 16;
static_assert(K2_CHUNK % K2_STAGE == 0 && K2_STAGE % K2_GK == 0, "a chunk is whole stages, a stage whole k-tiles");

static inline int kde2d_lds_bytes(int T) { return 8 * (4 * K2_GK * (T + K2_SKPAD) + 3 * K2_STAGE); }

static inline void kde2d_path_count(int path) { count_path(PATHS_KDE2D, path); }   // enum gpemu_kde2d_path

// the sheared second coordinate: THE expression of the density and of the extents
static __device__ __forceinline__ double shear_v(double beta, double x, double y) { return fma(-beta, x, y); }

// v = shear_v(beta, x, y) and lo with v + lo = y - beta x to second order: the product and the difference are split
// exactly (fma's residual, Knuth's two-sum) and recombined
static __device__ __forceinline__ double shear_v_lo(double beta, double x, double y, double v) {
#pragma clang fp contract(off)   // every operation below rounds on its own: a fused y - beta x would break the split
  const double p = beta * x, pe = fma(beta, x, -p);   // beta x = p + pe
  const double s = y - p, bb = s - y;                 // y - p = s + se
  const double se = (y - (s - bb)) - (p + bb);
  const double lo = ((s - v) + se) - pe;
  return lo == lo && fabs(lo) <= 0x1p-40 * fabs(v) ? lo : 0.0;   // (infinite or NaN inputs: v alone decides)
}

// one factor of the kernel: exp(-t^2 / 2); below -746 the exponential is exactly 0 in fp64; NaN stays NaN
static __device__ __forceinline__ double gauss_factor(double t) {
  const double e = -0.5 * (t * t);
  double f = 0.0;
  if (!(e < -746.0)) f = exp(e);
  return f;
}

struct Kde2dArgs {
  RowsView X;
  int64_t S, nchunk;
  int G, nt;                    // nt: tiles per axis
  const int *pairs;             // [pairs of the batch][2]
  const double *par;            // [..][3]: beta, 1 / h_a, 1 / h_b
  const double *ga, *gb;        // [..][G]
  double *part;                 // [..][nchunk][G][G]
};

// T: the side of the workgroup's tile, 64 or 128; the LDS is dynamic: kde2d_lds_bytes(T)
template <int T>
__global__ __launch_bounds__(256) void kde2d_partial_kernel(Kde2dArgs g) {
  constexpr int SK = T + K2_SKPAD;      // row length of an operand k-row in LDS
  constexpr int MI = T / 32;            // 16 x 16 tiles per axis of a wave's T/2 x T/2 quarter
  constexpr int NKG = 256 / T;          // threads per column of the generation: k-rows kg, kg + NKG, ...
  constexpr int NR = K2_GK / NKG;       // values of A and of B a thread generates per k-tile
  extern __shared__ __attribute__((aligned(16))) double k2_lds[];
  double *sA = k2_lds, *sB = sA + 2 * K2_GK * SK;                 // [2][GK * SK] each
  double *sx = sB + 2 * K2_GK * SK, *sv = sx + K2_STAGE, *svl = sv + K2_STAGE;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lk = lane >> 4;
  const int64_t c = blockIdx.x, p = blockIdx.z;
  const int ta = blockIdx.y / g.nt, tb = blockIdx.y % g.nt, G = g.G;
  const int pi = g.pairs[2 * p], pj = g.pairs[2 * p + 1];
  const double beta = g.par[3 * p], iha = g.par[3 * p + 1], ihb = g.par[3 * p + 2];

  // generation: this thread owns column gc of both operand tiles and the k-rows kg, kg + NKG, ... (kg is the same for
  // all lanes of a wave: the samples are read from LDS as broadcasts)
  const int gc = tid % T, kg = __builtin_amdgcn_readfirstlane(tid / T);
  const int ia = ta * T + gc, ib = tb * T + gc;
  const bool a_ok = ia < G, b_ok = ib < G;
  const double gav = a_ok ? g.ga[p * G + ia] : 0.0, gbv = b_ok ? g.gb[p * G + ib] : 0.0;
  double ra[NR], rb[NR];
  auto gen = [&](int kt) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int k = kt * K2_GK + kg + NKG * r;
      const double fa = gauss_factor((gav - sx[k]) * iha);
      const double fb = gauss_factor(((gbv - sv[k]) - svl[k]) * ihb);
      ra[r] = a_ok ? fa : 0.0;
      rb[r] = b_ok ? fb : 0.0;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      sA[buf * K2_GK * SK + (kg + NKG * r) * SK + gc] = ra[r];
      sB[buf * K2_GK * SK + (kg + NKG * r) * SK + gc] = rb[r];
    }
  };

  d4 acc[MI][MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < MI; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};

  const int64_t j0 = c * K2_CHUNK, j1 = (j0 + K2_CHUNK < g.S) ? j0 + K2_CHUNK : g.S;
  for (int64_t s0 = j0; s0 < j1; s0 += K2_STAGE) {
    // (the last k-tile of the previous stage ended in a barrier: sx, sv, svl and both operand buffers are free)
    {
      const int64_t r = s0 + tid;
      double x = INFINITY, v = INFINITY, vl = 0.0;   // a sample beyond the chunk: both factors are exactly 0
      if (r < j1) {
        const double *row = g.X.row(r);
        const double y = row[pj];
        x = row[pi];
        v = shear_v(beta, x, y);
        vl = shear_v_lo(beta, x, y, v);
      }
      sx[tid] = x;
      sv[tid] = v;
      svl[tid] = vl;
    }
    __syncthreads();
    const int n = (int)((j1 - s0 < K2_STAGE) ? j1 - s0 : K2_STAGE), nk = (n + K2_GK - 1) / K2_GK;
    gen(0);
    sstore(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int buf = kt & 1;
      const double *bA = sA + buf * K2_GK * SK, *bB = sB + buf * K2_GK * SK;
      if (kt + 1 < nk) gen(kt + 1);
#pragma unroll
      for (int ks = 0; ks < K2_GK / 4; ++ks) {
        double a[MI], b[MI];
        const int kk = ks * 4 + lk;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) a[mi] = bA[kk * SK + wm * (T / 2) + mi * 16 + lr];
#pragma unroll
        for (int ni = 0; ni < MI; ++ni) b[ni] = bB[kk * SK + wn * (T / 2) + ni * 16 + lr];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < MI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
      }
      if (kt + 1 < nk) sstore(buf ^ 1);
      __syncthreads();
    }
  }

  // D[reg] is row (lane >> 4) + 4 reg, column lane & 15 of each 16 x 16 tile; only the G x G part is stored
  double *out = g.part + (p * g.nchunk + c) * G * G;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < MI; ++ni) {
      const int col = tb * T + wn * (T / 2) + ni * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ta * T + wm * (T / 2) + mi * 16 + lk + 4 * r;
        if (row < G && col < G) out[(int64_t)row * G + col] = acc[mi][ni][r];
      }
    }
}

// dens[(p0 + p) G^2 + e] = norm[p] * (the element's partial tiles added in chunk order); thread (p, e)
__global__ __launch_bounds__(256) void kde2d_sum_kernel(const double *__restrict__ part, int64_t nchunk, int64_t GG,
                                                        int64_t n, const double *__restrict__ norm,
                                                        double *__restrict__ dens) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t p = i / GG, e = i % GG;
  const double *q = part + p * nchunk * GG + e;
  double s = 0.0;
  for (int64_t c = 0; c < nchunk; ++c) s += q[c * GG];
  dens[i] = s * norm[p];
}

// ---- pair moments (sums, minima and maxima over the workgroup: tree A of wg_dev.h) -----------------------------------
// mean == null: part[b][i] = the sum over the rows of block b of x_i (d entries); else part[b][e] = the sum of
// (x_i - mean_i) (x_j - mean_j), e over the pairs i <= j in row-major order (d (d + 1) / 2 entries)
__global__ __launch_bounds__(256) void pm_partial_kernel(RowsView v, const double *__restrict__ mean, int nent,
                                                         double *__restrict__ part) {
  __shared__ double red[256];
  const int t = threadIdx.x, d = v.d;
  const int64_t R = v.rows(), r0 = (int64_t)blockIdx.x * MOM_ROWS, r1 = (r0 + MOM_ROWS < R) ? r0 + MOM_ROWS : R;
  int e = 0;
  for (int i = 0; i < d; ++i) {
    const int jend = mean ? d : i + 1;
    const double mi = mean ? mean[i] : 0.0;
    for (int j = i; j < jend; ++j, ++e) {
      const double mj = mean ? mean[j] : 0.0;
      double s = 0.0;
      for (int64_t r = r0 + t; r < r1; r += 256) {
        const double *row = v.row(r);
        s += mean ? (row[i] - mi) * (row[j] - mj) : row[i];
      }
      s = wg_sum_a<256>(s, red);
      if (t == 0) part[(int64_t)blockIdx.x * nent + e] = s;
    }
  }
}

// dmean[d] = the pooled mean of the rows of v -- the first pass of pair_moments_rows, for other files (rows_dev.h);
// dpart: (rows + MOM_ROWS - 1) / MOM_ROWS * d doubles of scratch; asynchronous on st
int launch_pooled_mean(const RowsView &v, double *dpart, double *dmean, hipStream_t st) {
  const int64_t R = v.rows(), nb = (R + MOM_ROWS - 1) / MOM_ROWS;
  hipLaunchKernelGGL(pm_partial_kernel, dim3((unsigned)nb), dim3(256), 0, st, v, (const double *)nullptr, v.d, dpart);
  launch_moments_final(dpart, nb, v.d, R, dmean, st);
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

// part[(b P + p) 2 + {0, 1}] = the minimum and maximum of shear_v over the rows of block b; NaN is passed over (fmin,
// fmax)
__global__ __launch_bounds__(256) void pm_ext_partial_kernel(RowsView v, int P, const int *__restrict__ pairs,
                                                             const double *__restrict__ shear, double *__restrict__ part) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int64_t R = v.rows(), r0 = (int64_t)blockIdx.x * MOM_ROWS, r1 = (r0 + MOM_ROWS < R) ? r0 + MOM_ROWS : R;
  for (int p = 0; p < P; ++p) {
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    const double beta = shear[p];
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t r = r0 + t; r < r1; r += 256) {
      const double *row = v.row(r);
      const double w = shear_v(beta, row[i], row[j]);
      lo = fmin(lo, w);
      hi = fmax(hi, w);
    }
    lo = wg_min_a<256>(lo, red);
    hi = wg_max_a<256>(hi, red);
    if (t == 0) {
      part[((int64_t)blockIdx.x * P + p) * 2] = lo;
      part[((int64_t)blockIdx.x * P + p) * 2 + 1] = hi;
    }
  }
}

// ext[2 p + which] = the extreme over the blocks; workgroup (p, which)
__global__ __launch_bounds__(256) void pm_ext_final_kernel(const double *__restrict__ part, int64_t nb, int P,
                                                           double *__restrict__ ext) {
  __shared__ double red[256];
  const int e = blockIdx.x, which = e & 1;
  double s = which ? -INFINITY : INFINITY;
  for (int64_t b = threadIdx.x; b < nb; b += 256) {
    const double w = part[b * 2 * P + e];
    s = which ? fmax(s, w) : fmin(s, w);
  }
  s = which ? wg_max_a<256>(s, red) : wg_min_a<256>(s, red);
  if (threadIdx.x == 0) ext[e] = s;
}

// ---- host ------------------------------------------------------------------------------------------------------------
// the rows of the _dev calls as a view, within the limits of this file
static int kde2d_view(const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows, int d,
                      RowsView *v) {
  GP_ARG(dX, "null pointer");
  GP_ARG(d >= 1 && d <= K2_MAX_D, "d must be in [1, 16]");
  *v = RowsView{dX, n_blocks, block_rows, block_stride_rows * d, d};
  GP_TRY(rows_check(*v));
  GP_ARG(n_blocks <= ((1ll << 31) - 1) / block_rows, "S = n_blocks * block_rows must be in [1, 2^31)");
  return GPEMU_OK;
}

static int pairs_check(int d, int64_t P, const int64_t *pairs, const double *shear) {
  GP_ARG(pairs && shear, "null pointer");
  for (int64_t p = 0; p < P; ++p) {
    const int64_t i = pairs[2 * p], j = pairs[2 * p + 1];
    GP_ARG(i >= 0 && i < d && j >= 0 && j < d, "every pair index must be in [0, d)");
    GP_ARG(i != j, "the two parameters of a pair must differ");
    GP_ARG(std::isfinite(shear[p]), "every shear must be finite");
  }
  return GPEMU_OK;
}

static int kde2d_check(int d, int64_t P, const int64_t *pairs, const double *shear, const double *bw, int G,
                       const double *grid_a, const double *grid_b, const double *out, int64_t workspace_bytes) {
  GP_ARG(P >= 1 && P <= (1 << 20), "n_pairs must be in [1, 2^20]");
  GP_ARG(G >= 1 && G <= GPEMU_MAX_GRID_2D, "G must be in [1, 512]");
  GP_ARG(d >= 1 && d <= K2_MAX_D, "d must be in [1, 16]");
  GP_ARG(bw && grid_a && grid_b && out, "null pointer");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_TRY(pairs_check(d, P, pairs, shear));
  for (int64_t i = 0; i < 2 * P; ++i) GP_ARG(std::isfinite(bw[i]) && bw[i] > 0.0, "every bandwidth must be finite and > 0");
  for (int64_t i = 0; i < P * G; ++i)
    GP_ARG(std::isfinite(grid_a[i]) && std::isfinite(grid_b[i]), "grid points must be finite");
  return GPEMU_OK;
}

// the panels of device rows into ddens[P][G][G], in batches of pairs that fit workspace_bytes; waits for st
static int kde2d_rows(const RowsView &X, int64_t P, const int64_t *pairs, const double *shear, const double *bw, int G,
                      const double *grid_a, const double *grid_b, double *ddens, int64_t workspace_bytes, hipStream_t st) {
  const int64_t S = X.rows(), nchunk = (S + K2_CHUNK - 1) / K2_CHUNK, GG = (int64_t)G * G;
  const int T = G <= K2_T_SMALL ? K2_T_SMALL : K2_T, nt = (G + T - 1) / T;
  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t per_pair = 8 * GG * nchunk;
  const int64_t cap = std::min<int64_t>(std::min<int64_t>(P, budget / per_pair), 65535);
  if (cap < 1) {
    set_error("kde2d: out of memory: the partial tiles of one pair (%lld samples, G = %d) need %lld bytes; %lld bytes %s",
              (long long)S, G, (long long)per_pair, (long long)budget, workspace_budget_name(workspace_bytes));
    return GPEMU_ERR_HIP;
  }
  std::vector<int> hp((size_t)(2 * P));
  std::vector<double> par((size_t)(3 * P)), norm((size_t)P);
  for (int64_t p = 0; p < P; ++p) {
    hp[(size_t)(2 * p)] = (int)pairs[2 * p];
    hp[(size_t)(2 * p + 1)] = (int)pairs[2 * p + 1];
    par[(size_t)(3 * p)] = shear[p];
    par[(size_t)(3 * p + 1)] = 1.0 / bw[2 * p];
    par[(size_t)(3 * p + 2)] = 1.0 / bw[2 * p + 1];
    norm[(size_t)p] = 1.0 / ((((double)S * (2.0 * M_PI)) * bw[2 * p]) * bw[2 * p + 1]);
  }
  GP_TRY(allow_dynamic_lds((const void *)kde2d_partial_kernel<K2_T>, kde2d_lds_bytes(K2_T)));
  DevScope sc(st);
  int *dpairs = nullptr;
  double *dpar = nullptr, *dnorm = nullptr, *dga = nullptr, *dgb = nullptr, *part = nullptr;
  GP_TRY(sc.alloc(&dpairs, 2 * P));
  GP_TRY(sc.alloc(&dpar, 3 * P));
  GP_TRY(sc.alloc(&dnorm, P));
  GP_TRY(sc.alloc(&dga, P * G));
  GP_TRY(sc.alloc(&dgb, P * G));
  GP_TRY(sc.alloc(&part, cap * nchunk * GG));
  GP_TRY(upload(dpairs, hp.data(), 2 * P, st));
  GP_TRY(upload(dpar, par.data(), 3 * P, st));
  GP_TRY(upload(dnorm, norm.data(), P, st));
  GP_TRY(upload(dga, grid_a, P * G, st));
  GP_TRY(upload(dgb, grid_b, P * G, st));
  Kde2dArgs a;
  a.X = X; a.S = S; a.nchunk = nchunk; a.G = G; a.nt = nt; a.part = part;
  for (int64_t p0 = 0; p0 < P; p0 += cap) {
    const int64_t np = std::min(cap, P - p0);
    a.pairs = dpairs + 2 * p0; a.par = dpar + 3 * p0; a.ga = dga + p0 * G; a.gb = dgb + p0 * G;
    kde2d_path_count(GPEMU_KDE2D_PATH_PAIR_BATCH);
    kde2d_path_count(GPEMU_KDE2D_PATH_DENSITY);
    const dim3 grid((unsigned)nchunk, (unsigned)(nt * nt), (unsigned)np);
    if (T == K2_T_SMALL)
      hipLaunchKernelGGL(kde2d_partial_kernel<K2_T_SMALL>, grid, dim3(256), kde2d_lds_bytes(K2_T_SMALL), st, a);
    else
      hipLaunchKernelGGL(kde2d_partial_kernel<K2_T>, grid, dim3(256), kde2d_lds_bytes(K2_T), st, a);
    GP_HIP(hipGetLastError());
    kde2d_path_count(GPEMU_KDE2D_PATH_PARTIAL_SUM);
    hipLaunchKernelGGL(kde2d_sum_kernel, dim3((unsigned)((np * GG + 255) / 256)), dim3(256), 0, st, (const double *)part,
                       nchunk, GG, np * GG, (const double *)(dnorm + p0), ddens + p0 * GG);
    GP_HIP(hipGetLastError());
  }
  GP_HIP(hipStreamSynchronize(st));   // the host vectors are read by the copies above
  return GPEMU_OK;
}

static int pair_moments_rows(const RowsView &X, double *mean, double *cov, int64_t P, const int64_t *pairs,
                             const double *shear, double *ext, hipStream_t st) {
  const int d = X.d;
  const int64_t R = X.rows(), nb = (R + MOM_ROWS - 1) / MOM_ROWS;
  const int ncov = d * (d + 1) / 2;
  DevScope sc(st);
  double *dpart = nullptr, *dmean = nullptr, *dcov = nullptr, *dshear = nullptr, *dext = nullptr;
  int *dpairs = nullptr;
  std::vector<double> tri((size_t)ncov);
  std::vector<int> hp((size_t)(2 * P));
  GP_TRY(sc.alloc(&dpart, nb * std::max<int64_t>(ncov, 2 * P)));
  if (mean) {
    kde2d_path_count(GPEMU_KDE2D_PATH_MOMENTS);
    GP_TRY(sc.alloc(&dmean, d));
    GP_TRY(sc.alloc(&dcov, ncov));
    hipLaunchKernelGGL(pm_partial_kernel, dim3((unsigned)nb), dim3(256), 0, st, X, (const double *)nullptr, d, dpart);
    launch_moments_final(dpart, nb, d, R, dmean, st);
    hipLaunchKernelGGL(pm_partial_kernel, dim3((unsigned)nb), dim3(256), 0, st, X, (const double *)dmean, ncov, dpart);
    launch_moments_final(dpart, nb, ncov, R, dcov, st);
    GP_HIP(hipGetLastError());
    GP_TRY(sc.download(mean, dmean, d));
    GP_TRY(sc.download(tri.data(), dcov, ncov));
  }
  if (P > 0) {
    kde2d_path_count(GPEMU_KDE2D_PATH_EXTENTS);
    for (int64_t i = 0; i < 2 * P; ++i) hp[(size_t)i] = (int)pairs[i];
    GP_TRY(sc.alloc(&dpairs, 2 * P));
    GP_TRY(sc.alloc(&dshear, P));
    GP_TRY(sc.alloc(&dext, 2 * P));
    GP_TRY(upload(dpairs, hp.data(), 2 * P, st));
    GP_TRY(upload(dshear, shear, P, st));
    hipLaunchKernelGGL(pm_ext_partial_kernel, dim3((unsigned)nb), dim3(256), 0, st, X, (int)P, (const int *)dpairs,
                       (const double *)dshear, dpart);
    hipLaunchKernelGGL(pm_ext_final_kernel, dim3((unsigned)(2 * P)), dim3(256), 0, st, (const double *)dpart, nb, (int)P,
                       dext);
    GP_HIP(hipGetLastError());
    GP_TRY(sc.download(ext, dext, 2 * P));
  }
  GP_HIP(hipStreamSynchronize(st));
  if (mean)
    for (int i = 0, e = 0; i < d; ++i)
      for (int j = i; j < d; ++j, ++e) cov[i * d + j] = cov[j * d + i] = tri[(size_t)e];
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_kde2d_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_KDE2D, out, n); }

int gpemu_kde2d_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows, int d,
                    int64_t n_pairs, const int64_t *pairs, const double *shear, const double *bandwidth, int G,
                    const double *grid_a, const double *grid_b, double *dout, int64_t workspace_bytes, void *stream) {
  GP_TRY(kde2d_check(d, n_pairs, pairs, shear, bandwidth, G, grid_a, grid_b, dout, workspace_bytes));
  RowsView X;
  GP_TRY(kde2d_view(dX, n_blocks, block_rows, block_stride_rows, d, &X));
  GP_TRY(device_ready(device));
  return kde2d_rows(X, n_pairs, pairs, shear, bandwidth, G, grid_a, grid_b, dout, workspace_bytes, (hipStream_t)stream);
}

int gpemu_kde2d(int device, int64_t S, int d, const double *X, int64_t n_pairs, const int64_t *pairs, const double *shear,
                const double *bandwidth, int G, const double *grid_a, const double *grid_b, double *out,
                int64_t workspace_bytes) {
  GP_TRY(kde2d_check(d, n_pairs, pairs, shear, bandwidth, G, grid_a, grid_b, out, workspace_bytes));
  GP_ARG(X, "null pointer");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  const int64_t n = n_pairs * G * G;
  DevScope sc(st);
  double *dX = nullptr, *dout = nullptr;
  GP_TRY(sc.alloc(&dX, S * d));
  GP_TRY(sc.alloc(&dout, n));
  GP_TRY(upload(dX, X, S * d, st));
  GP_TRY(kde2d_rows(RowsView{dX, 1, S, S * d, d}, n_pairs, pairs, shear, bandwidth, G, grid_a, grid_b, dout,
                    workspace_bytes, st));
  GP_TRY(sc.download(out, dout, n));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_pair_moments_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows,
                           int d, double *mean, double *cov, int64_t n_pairs, const int64_t *pairs, const double *shear,
                           double *ext, void *stream) {
  RowsView X;
  GP_TRY(kde2d_view(dX, n_blocks, block_rows, block_stride_rows, d, &X));
  GP_ARG((mean == nullptr) == (cov == nullptr), "mean and cov go together");
  GP_ARG(n_pairs >= 0 && n_pairs <= (1 << 20), "n_pairs must be in [0, 2^20]");
  GP_ARG(mean || n_pairs > 0, "nothing to compute");
  if (n_pairs > 0) {
    GP_ARG(ext, "null pointer");
    GP_TRY(pairs_check(d, n_pairs, pairs, shear));
  }
  GP_TRY(device_ready(device));
  return pair_moments_rows(X, mean, cov, n_pairs, pairs, shear, ext, (hipStream_t)stream);
}

}  // extern "C"
