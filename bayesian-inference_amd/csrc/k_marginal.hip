// Marginal posteriors of a stored chain (gpemu_marginal_hist*, gpemu_hpd*, gpemu_kde1d*): the data of a
// corner plot from every sample, where the chain lies.
//
// Histograms (hist_*; also what gpemu_weighted_hist* of k_reweight.hip runs, through hist_rows of rows_dev.h; DESIGN
// 4.40): one sweep of hist_sweep_kernel over the rows fills, per workgroup, private bins in LDS for the 1-D histograms of
// parameters [a0, a1) and the 2-D histograms of pairs [p0, p1).  A thread owns a row: its d doubles are loaded once,
// every bin index is found once (guessed from the affine map of the box, then walked to the bin whose edges hold the
// value: numpy's rule, on the edges themselves) and shared by all pairs of the sweep.  Non-zero bins go to the 64-bit
// outputs with global integer atomics.  The kernel is written once; a bin policy gives the two forms:
//   Bins16  counted: 16-bit counters, two to a 32-bit word, advanced by LDS integer atomics of 1 or 1 << 16; a workgroup
//           takes at most HS_MAX_ROWS16 < 2^16 rows, so a counter cannot carry into its neighbour.  73728 to a sweep;
//   Bins64  weighted: 64-bit bins that take the row's integer weight q[w][s] (a row of weight 0 is skipped); 18432 to a
//           sweep, grid.y = the weight row.
// The host plans the sweeps: floor(cap / nb2^2) pairs each, or, where the nb2^2 bins of a pair do not fit, one pair in
// bands of its first index; the 1-D bins beside the last sweep of pairs where they fit, else in sweeps of their own.
// Every bin is an integer: nothing depends on the grid, on the plan or on the run.
//
// Highest-density intervals (hpd_*): the rows are sorted by k_rows.hip's radix sort in batches; hpd_window_kernel takes,
// for every (row, level, chunk of HW_PER windows), the lexicographic minimum of (s[S - n + i] - s[i], i), and
// hpd_finish_kernel that of a (row, level)'s chunks: the narrowest window, the smallest i among ties (np.argmin).
//
// Kernel density (kde_*): workgroup (chunk of KD_CHUNK samples, tile of 256 GPT grid points, row).  A thread keeps GPT
// grid points in registers; the samples go through LDS in stages of KD_STAGE and sample j of the chunk is added to sum
// j mod 4 of every grid point, so the order of every sum is fixed by the sample index.  kde_sum_kernel adds a grid
// point's chunk sums: lane-strided in chunk order, then tree B of wg_dev.h.  A term whose exponent is below -746 is
// exactly 0 in fp64 and is not evaluated.
//
// Under the fixed-point weights of a reweighted chain (gpemu_weighted_hpd*, gpemu_weighted_kde1d*): the
// intervals by value (whpd_*: the same sort, the weights placed at the first sorted position of their key with integer
// atomics, a three-launch 64-bit prefix sum, a bisection per run start, the same lexicographic reduction) and the
// density with (double)q exp(.) as its term (kde_partial_kernel's KdeFixed instance; the unweighted one is KdeUnit).
#include <algorithm>
#include <cmath>
#include <vector>

#include "internal.h"
#include "rows_dev.h"
#include "sampler_internal.h"
#include "wg_dev.h"

namespace gpemu {

constexpr int HS_THREADS = 1024;
constexpr int64_t HS_MAX_ROWS16 = 65280; // rows per workgroup of a counted sweep, < 2^16: a 16-bit counter cannot overflow
constexpr int HW_PER = 4096;             // windows per workgroup of the window search
constexpr int KD_CHUNK = 8192;           // samples per partial sum
constexpr int KD_STAGE = 1024;           // samples staged in LDS at a time
constexpr int KD_MAX_GPT = 4;            // grid points per thread: tiles of up to 1024 grid points
constexpr int64_t KD_PART_BYTES = 256ll << 20;   // chunk sums of a batch of rows, about

static inline void marginal_path_count(int path) { count_path(PATHS_MARGINAL, path); }   // enum gpemu_marginal_path

// ---- histograms ----------------------------------------------------------------------------------------------------
struct HistArgs {
  RowsView X;
  int64_t S, rows_per_wg;
  const u64 *q;                    // [R_w][ldq]; not read by the counted form
  int64_t ldq;
  const double *e1, *e2;           // [d][nb1 + 1], [d][nb2 + 1]
  int nb1, nb2;
  int a0, a1, p0, p1;              // this sweep: 1-D histograms of parameters [a0, a1), pairs [p0, p1)
  int i0, j0;                      // pair p0 = (i0, j0)
  int band0, band;                 // ... of the pairs, the bins [band0, band0 + band) of the first index: all nb2 of them,
                                   // or a band of ONE pair -- either way one contiguous piece of hist2
  u64 *hist1, *hist2;              // [R_w][d][nb1], [R_w][np][nb2][nb2]
  int64_t n1_all, n2_all;          // d nb1, np nb2^2
};

// the bin b with e[b] <= x < e[b + 1], the last one closed on the right; -1 outside [e[0], e[nb]] and for NaN.
// tab = {e[0], e[nb], nb / (e[nb] - e[0])}
static __device__ __forceinline__ int hist_bin(double x, const double *__restrict__ e, int nb, const double *tab) {
  const double e0 = tab[0], eN = tab[1];
  if (!(x >= e0 && x <= eN)) return -1;
  double t = (x - e0) * tab[2];
  t = fmin(fmax(t, 0.0), (double)(nb - 1));   // a NaN guess (an infinite span) starts at 0
  int b = (int)t;
  while (b > 0 && x < e[b]) --b;
  while (b < nb - 1 && x >= e[b + 1]) ++b;
  return b;
}

// The bins of a workgroup in LDS.  Counted: 16-bit counters, two to a word, that take 1 per row.
struct Bins16 {
  typedef unsigned word;
  static constexpr bool weighted = false;
  static __device__ __forceinline__ int words(int n) { return (n + 1) >> 1; }
  static __device__ __forceinline__ void add(word *lds, int c, u64) { atomicAdd(&lds[c >> 1], 1u << ((c & 1) << 4)); }
  template <class F>   // f(bin, value) for the non-zero bins below n of word w
  static __device__ __forceinline__ void flush(word v, int w, int n, F f) {
    if (!v) return;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int c = 2 * w + half;
      const unsigned cnt = (v >> (16 * half)) & 0xffffu;
      if (cnt && c < n) f(c, (u64)cnt);
    }
  }
};
// Weighted: 64-bit bins that take the row's weight.
struct Bins64 {
  typedef u64 word;
  static constexpr bool weighted = true;
  static __device__ __forceinline__ int words(int n) { return n; }
  static __device__ __forceinline__ void add(word *lds, int c, u64 wt) { atomicAdd(&lds[c], wt); }
  template <class F>
  static __device__ __forceinline__ void flush(word v, int w, int, F f) {
    if (v) f(w, v);
  }
};

// workgroup (rows [x rows_per_wg, (x + 1) rows_per_wg), weight row y)
template <int DP, class Bins>
__global__ __launch_bounds__(HS_THREADS) void hist_sweep_kernel(HistArgs a) {
  extern __shared__ __align__(8) unsigned char hs_lds[];   // the bins: 1-D section, then the pairs (their bands)
  __shared__ double tab[2][ROWS_MAX_D][3];
  typename Bins::word *lds = (typename Bins::word *)hs_lds;
  const int tid = threadIdx.x;
  const int d = a.X.d, nb1 = a.nb1, nb2 = a.nb2, psz = a.band * nb2;
  const int n1 = (a.a1 - a.a0) * nb1, nbins = n1 + (a.p1 - a.p0) * psz, nwords = Bins::words(nbins);
  for (int w = tid; w < nwords; w += HS_THREADS) lds[w] = 0;
  if (tid < 2 * d) {
    const int which = tid / d, k = tid % d, nb = which ? nb2 : nb1;
    const double *e = (which ? a.e2 : a.e1) + (int64_t)k * (nb + 1);
    tab[which][k][0] = e[0];
    tab[which][k][1] = e[nb];
    tab[which][k][2] = (double)nb / (e[nb] - e[0]);
  }
  __syncthreads();
  const u64 *qrow = a.q + (int64_t)blockIdx.y * a.ldq;
  const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_wg, r1 = (r0 + a.rows_per_wg < a.S) ? r0 + a.rows_per_wg : a.S;
  for (int64_t r = r0 + tid; r < r1; r += HS_THREADS) {
    u64 wt = 1;
    if (Bins::weighted) {
      wt = qrow[r];
      if (wt == 0) continue;
    }
    const double *row = a.X.row(r);
    u64 pk[DP / 4];   // the 2-D bins + 1 (0: outside), 16 bits each: k is uniform, a select per word keeps them in registers
#pragma unroll
    for (int w = 0; w < DP / 4; ++w) pk[w] = 0;
#pragma unroll 1
    for (int k = 0; k < d; ++k) {
      const double xv = row[k];
      if (k >= a.a0 && k < a.a1) {
        const int b = hist_bin(xv, a.e1 + (int64_t)k * (nb1 + 1), nb1, tab[0][k]);
        if (b >= 0) Bins::add(lds, (k - a.a0) * nb1 + b, wt);
      }
      if (a.p1 > a.p0) {
        const u64 b = (u64)(hist_bin(xv, a.e2 + (int64_t)k * (nb2 + 1), nb2, tab[1][k]) + 1) << ((k & 3) * 16);
#pragma unroll
        for (int w = 0; w < DP / 4; ++w) pk[w] |= (w == (k >> 2)) ? b : 0;
      }
    }
    if (a.p1 > a.p0) {
      int i = a.i0, j = a.j0, off = n1;   // pair p0 = (i0, j0), then row-major: the index is the same for every lane
#pragma unroll 1
      for (int p = a.p0; p < a.p1; ++p) {
        u64 wi = 0, wj = 0;
#pragma unroll
        for (int w = 0; w < DP / 4; ++w) {
          wi = (w == (i >> 2)) ? pk[w] : wi;
          wj = (w == (j >> 2)) ? pk[w] : wj;
        }
        int bi = (int)((wi >> ((i & 3) * 16)) & 0xffff) - 1;
        const int bj = (int)((wj >> ((j & 3) * 16)) & 0xffff) - 1;
        bi -= a.band0;
        if (bi >= 0 && bi < a.band && bj >= 0) Bins::add(lds, off + bi * nb2 + bj, wt);
        off += psz;
        if (++j == d) {
          ++i;
          j = i + 1;
        }
      }
    }
  }
  __syncthreads();
  u64 *g1 = a.hist1 + (int64_t)blockIdx.y * a.n1_all + (int64_t)a.a0 * nb1;
  u64 *g2 = a.hist2 + (int64_t)blockIdx.y * a.n2_all + ((int64_t)a.p0 * nb2 + a.band0) * nb2;
  for (int w = tid; w < nwords; w += HS_THREADS)
    Bins::flush(lds[w], w, nbins, [&](int c, u64 v) { atomicAdd(c < n1 ? &g1[c] : &g2[c - n1], v); });
}

// inside[w d + j] = the sum of hist1[w][j][.]; workgroup w d + j
__global__ __launch_bounds__(256) void hist_inside_kernel(const u64 *__restrict__ hist1, int nb1, u64 *__restrict__ inside) {
  __shared__ u64 red[256];
  const int tid = threadIdx.x;
  u64 s = 0;
  for (int b = tid; b < nb1; b += 256) s += hist1[(int64_t)blockIdx.x * nb1 + b];
  s = wg_sum_a<256>(s, red);
  if (tid == 0) inside[blockIdx.x] = s;
}

struct HistSweep { int a0, a1, p0, p1, band0, band; };

// the sweeps of one call; cap: bins per sweep.  nb2^2 <= cap: floor(cap / nb2^2) whole pairs per sweep; nb2^2 > cap: one
// pair per sweep, in bands of floor(cap / nb2) bins of its first index.  The 1-D bins beside the last sweep of pairs where
// they fit, else in sweeps of their own
static std::vector<HistSweep> hist_plan(int d, int nb1, int nb2, int64_t cap) {
  std::vector<HistSweep> plan;
  const int np = d * (d - 1) / 2;
  const int64_t sq = (int64_t)nb2 * nb2, dpg = cap / nb1;
  if (sq <= cap) {
    const int64_t ppg = cap / sq;
    for (int p0 = 0; p0 < np; p0 += (int)ppg) plan.push_back({0, 0, p0, (int)std::min<int64_t>(np, p0 + ppg), 0, nb2});
  } else {
    const int band = (int)(cap / nb2);
    for (int p = 0; p < np; ++p)
      for (int b0 = 0; b0 < nb2; b0 += band) plan.push_back({0, 0, p, p + 1, b0, std::min(band, nb2 - b0)});
  }
  int a = 0;
  if (!plan.empty()) {   // beside the last sweep of pairs, as many parameters as fit
    HistSweep &last = plan.back();
    a = (int)std::min<int64_t>(d, (cap - (int64_t)(last.p1 - last.p0) * last.band * nb2) / nb1);
    last.a1 = a;
  }
  for (; a < d; a += (int)dpg) plan.push_back({a, (int)std::min<int64_t>(d, a + dpg), 0, 0, 0, nb2});
  return plan;
}

int edges_check(const double *e, int d, int nb) {
  for (int k = 0; k < d; ++k)
    for (int b = 0; b <= nb; ++b) {
      const double v = e[(int64_t)k * (nb + 1) + b];
      GP_ARG(std::isfinite(v), "bin edges must be finite");
      GP_ARG(b == 0 || v > e[(int64_t)k * (nb + 1) + b - 1], "bin edges must be strictly increasing");
    }
  return GPEMU_OK;
}

int hist_rows(const RowsView &X, int64_t R_w, const u64 *dq, int64_t ldq, int nb1, const double *edges1, int nb2,
              const double *edges2, int64_t cap, u64 *dhist1, u64 *dhist2, u64 *dinside1, void (*on_sweep)(bool pairs),
              hipStream_t st) {
  const int d = X.d;
  const int64_t S = X.rows(), np = d * (d - 1) / 2;
  const std::vector<HistSweep> plan = hist_plan(d, nb1, nb2, cap);
  DevScope sc(st);
  double *de1 = nullptr, *de2 = nullptr;
  GP_TRY(sc.alloc(&de1, (int64_t)d * (nb1 + 1)));
  GP_TRY(sc.alloc(&de2, (int64_t)d * (nb2 + 1)));
  GP_TRY(upload(de1, edges1, (int64_t)d * (nb1 + 1), st));
  GP_TRY(upload(de2, edges2, (int64_t)d * (nb2 + 1), st));
  HistArgs a;
  a.X = X; a.S = S; a.q = dq; a.ldq = ldq;
  a.rows_per_wg = std::max<int64_t>(4096, round_up((S + 1023) / 1024, 256));
  if (!dq) a.rows_per_wg = std::min(a.rows_per_wg, HS_MAX_ROWS16);
  a.e1 = de1; a.e2 = de2; a.nb1 = nb1; a.nb2 = nb2;
  a.hist1 = dhist1; a.hist2 = dhist2;
  a.n1_all = (int64_t)d * nb1; a.n2_all = np * nb2 * nb2;
  GP_HIP(hipMemsetAsync(dhist1, 0, sizeof(u64) * (size_t)(R_w * a.n1_all), st));
  if (np > 0) GP_HIP(hipMemsetAsync(dhist2, 0, sizeof(u64) * (size_t)(R_w * a.n2_all), st));
  const dim3 grid((unsigned)((S + a.rows_per_wg - 1) / a.rows_per_wg), (unsigned)R_w);
  void (*const fn)(HistArgs) = dq ? (d <= 8 ? hist_sweep_kernel<8, Bins64> : hist_sweep_kernel<16, Bins64>)
                                  : (d <= 8 ? hist_sweep_kernel<8, Bins16> : hist_sweep_kernel<16, Bins16>);
  GP_TRY(allow_dynamic_lds((const void *)fn, (int)(dq ? 8 * HIST_CAP64 : 2 * HIST_CAP16 + 16)));
  for (const HistSweep &sw : plan) {
    a.a0 = sw.a0; a.a1 = sw.a1; a.p0 = sw.p0; a.p1 = sw.p1; a.band0 = sw.band0; a.band = sw.band;
    int i0 = 0, rem = sw.p0;   // row i of the pair list holds d - 1 - i pairs
    while (i0 < d - 1 && rem >= d - 1 - i0) rem -= d - 1 - i0++;
    a.i0 = i0; a.j0 = i0 + 1 + rem;
    const int64_t nbins = (int64_t)(sw.a1 - sw.a0) * nb1 + (int64_t)(sw.p1 - sw.p0) * sw.band * nb2;
    const size_t lds = dq ? (size_t)(8 * std::max<int64_t>(nbins, 1)) : (size_t)round_up(2 * nbins + 2, 16);
    on_sweep(sw.p1 > sw.p0);
    hipLaunchKernelGGL(fn, grid, dim3(HS_THREADS), lds, st, a);
    GP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(hist_inside_kernel, dim3((unsigned)(R_w * d)), dim3(256), 0, st, (const u64 *)dhist1, nb1, dinside1);
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(st));   // the edges are read by the copies above
  return GPEMU_OK;
}

static int hist_check(int d, int nb1, const double *edges1, int nb2, const double *edges2, int64_t group_counters,
                      const void *hist1, const void *hist2, const void *n_inside1) {
  GP_ARG(d >= 1 && d <= ROWS_MAX_D, "d must be in [1, 16]");
  GP_ARG(nb1 >= 1 && nb1 <= 4096, "nb1 must be in [1, 4096]");
  GP_ARG(nb2 >= 1 && nb2 <= 256, "nb2 must be in [1, 256]");
  GP_ARG(edges1 && edges2 && hist1 && n_inside1 && (hist2 || d == 1), "null pointer");
  GP_ARG(group_counters == 0 || (group_counters >= std::max<int64_t>(nb1, (int64_t)nb2 * nb2) && group_counters <= HIST_CAP16),
         "group_counters must be 0 or in [max(nb1, nb2^2), 73728]");
  GP_TRY(edges_check(edges1, d, nb1));
  GP_TRY(edges_check(edges2, d, nb2));
  return GPEMU_OK;
}

// the counted sweep over device rows; waits for st
static int count_rows(const RowsView &X, int nb1, const double *edges1, int nb2, const double *edges2,
                      int64_t group_counters, int64_t *dhist1, int64_t *dhist2, int64_t *dn_inside1, hipStream_t st) {
  return hist_rows(X, 1, nullptr, 0, nb1, edges1, nb2, edges2, group_counters ? group_counters : HIST_CAP16, (u64 *)dhist1,
                   (u64 *)dhist2, (u64 *)dn_inside1, [](bool pairs) {
                     marginal_path_count(GPEMU_MARGINAL_PATH_HIST_SWEEP);
                     if (pairs) marginal_path_count(GPEMU_MARGINAL_PATH_PAIR_GROUP);
                   }, st);
}

// ---- highest-density intervals ---------------------------------------------------------------------------------------
// is (w, i) before (bw, bi) in the lexicographic order?
static __device__ __forceinline__ bool hpd_before(double w, long long i, double bw, long long bi) {
  return w < bw || (w == bw && i < bi);
}

// the lexicographic minimum over the workgroup, valid in thread 0
static __device__ __forceinline__ void hpd_wg_min(double &w, long long &i, double *sw, long long *si) {
  const int tid = threadIdx.x;
  sw[tid] = w;
  si[tid] = i;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off && hpd_before(sw[tid + off], si[tid + off], sw[tid], si[tid])) {
      sw[tid] = sw[tid + off];
      si[tid] = si[tid + off];
    }
    __syncthreads();
  }
  w = sw[0];
  i = si[0];
}

// pw / pi[(rl L + l) nchunk + c] = the minimum of (s[S - n + i] - s[i], i) over the windows i of chunk c, i < n = n_out[l]
__global__ __launch_bounds__(256) void hpd_window_kernel(const u64 *__restrict__ sorted, int64_t S, int n_levels,
                                                         const int64_t *__restrict__ n_out, int64_t nchunk,
                                                         double *__restrict__ pw, long long *__restrict__ pi) {
  __shared__ double sw[256];
  __shared__ long long si[256];
  const int64_t c = blockIdx.x % nchunk, rl_l = blockIdx.x / nchunk, rl = rl_l / n_levels;
  const int64_t n = n_out[rl_l % n_levels];
  const u64 *k = sorted + rl * S;
  double bw = INFINITY;
  long long bi = 0x7fffffffffffffffll;
#pragma unroll 4
  for (int j = 0; j < HW_PER / 256; ++j) {
    const int64_t i = c * HW_PER + (int64_t)j * 256 + threadIdx.x;
    if (i < n) {
      const double w = sel_value(k[S - n + i]) - sel_value(k[i]);
      if (hpd_before(w, i, bw, bi)) { bw = w; bi = i; }
    }
  }
  hpd_wg_min(bw, bi, sw, si);
  if (threadIdx.x == 0) {
    pw[blockIdx.x] = bw;
    pi[blockIdx.x] = bi;
  }
}

// out[((row0 + rl) L + l) 2 + {0, 1}] = the ends of the narrowest window; workgroup (rl, l)
__global__ __launch_bounds__(256) void hpd_finish_kernel(const u64 *__restrict__ sorted, int64_t S, int n_levels,
                                                         const int64_t *__restrict__ n_out, int64_t nchunk,
                                                         const double *__restrict__ pw, const long long *__restrict__ pi,
                                                         const int *__restrict__ nan, int64_t row0,
                                                         double *__restrict__ out) {
  __shared__ double sw[256];
  __shared__ long long si[256];
  const int64_t rl = blockIdx.x / n_levels;
  const int64_t n = n_out[blockIdx.x % n_levels];
  double bw = INFINITY;
  long long bi = 0x7fffffffffffffffll;
  for (int64_t c = threadIdx.x; c < nchunk; c += 256) {
    const double w = pw[(int64_t)blockIdx.x * nchunk + c];
    const long long i = pi[(int64_t)blockIdx.x * nchunk + c];
    if (hpd_before(w, i, bw, bi)) { bw = w; bi = i; }
  }
  hpd_wg_min(bw, bi, sw, si);
  if (threadIdx.x == 0) {
    const u64 *k = sorted + rl * S;
    const double smin = sel_value(k[0]), smax = sel_value(k[S - 1]);
    double lo = sel_nan(), hi = lo;
    // (a chunk's sentinel index survives only where every width is a NaN: a row with an infinite end)
    if (!nan[rl] && !isinf(smin) && !isinf(smax) && bi >= 0 && bi < n) {
      lo = sel_value(k[bi]);
      hi = sel_value(k[S - n + bi]);
    }
    double *o = out + ((row0 + rl) * n_levels + blockIdx.x % n_levels) * 2;
    o[0] = lo;
    o[1] = hi;
  }
}

static int hpd_check(int64_t R, int64_t S, int64_t n_levels, const int64_t *n_out) {
  GP_ARG(R > 0, "R must be positive");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(n_levels > 0 && n_levels <= 4096 && n_out, "n_levels must be in [1, 4096]");
  for (int64_t l = 0; l < n_levels; ++l) GP_ARG(n_out[l] >= 1 && n_out[l] <= S, "every n_out must be in [1, S]");
  return GPEMU_OK;
}

// the intervals of R rows, in batches of rows that fit workspace_bytes (0: half of the free memory); waits for st
static int hpd_rows(const double *dV, int64_t R, int64_t S, int64_t row_stride, int64_t elem_stride, int64_t n_levels,
                    const int64_t *n_out, double *dout, int64_t workspace_bytes, hipStream_t st) {
  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t n_max = *std::max_element(n_out, n_out + n_levels), nchunk = (n_max + HW_PER - 1) / HW_PER;
  const int64_t per_row = rank_row_bytes(S) + 16 * n_levels * nchunk;   // the sort's and the windows' (pw, pi)
  const int64_t rows_cap = sort_rows_cap(R, S, budget, per_row, n_levels * nchunk);
  if (rows_cap < 1) {
    set_error("hpd: out of memory: one row of %lld elements and %lld levels needs %lld bytes of sort and window buffers; "
              "%lld bytes %s", (long long)S, (long long)n_levels, (long long)per_row, (long long)budget,
              workspace_budget_name(workspace_bytes));
    return GPEMU_ERR_HIP;
  }
  DevScope sc(st);
  SortScratch sort;
  int64_t *dn = nullptr;
  double *pw = nullptr;
  long long *pi = nullptr;
  GP_TRY(sort.alloc(sc, rows_cap, S));
  GP_TRY(sc.alloc(&dn, n_levels));
  GP_TRY(sc.alloc(&pw, rows_cap * n_levels * nchunk));
  GP_TRY(sc.alloc(&pi, rows_cap * n_levels * nchunk));
  GP_TRY(upload(dn, n_out, n_levels, st));
  for (int64_t row0 = 0; row0 < R; row0 += rows_cap) {
    const int64_t rows = std::min(rows_cap, R - row0);
    marginal_path_count(GPEMU_MARGINAL_PATH_SORT_BATCH);
    GP_TRY(sort_rows(dV, row_stride, elem_stride, S, row0, rows, sort, [] {}, st));
    marginal_path_count(GPEMU_MARGINAL_PATH_WINDOW_SEARCH);
    hipLaunchKernelGGL(hpd_window_kernel, dim3((unsigned)(rows * n_levels * nchunk)), dim3(256), 0, st, sort.ka, S,
                       (int)n_levels, dn, nchunk, pw, pi);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(hpd_finish_kernel, dim3((unsigned)(rows * n_levels)), dim3(256), 0, st, sort.ka, S, (int)n_levels, dn,
                       nchunk, pw, pi, sort.nan, row0, dout);
    GP_HIP(hipGetLastError());
  }
  GP_HIP(hipStreamSynchronize(st));   // n_out is read by the copy above
  return GPEMU_OK;
}

// ---- weighted highest-density intervals (gpemu_weighted_hpd*) --------------------------------------------
// For sorted keys k[0 .. S) of a value row and the weights of a weight row placed at the first position of their key, C
// their inclusive prefix sum: the interval of target mass t that starts at run start i (k[i] != k[i - 1]) ends at the
// first j >= i with C[j] - C[i - 1] >= t, and the answer is the lexicographic minimum of (k[j] - k[i], i).
constexpr int WH_SCAN = 2048;   // positions per workgroup of the prefix sum: 8 to a thread

// the first position of `key` in the sorted row k[0 .. S); every key looked up is in the row
static __device__ __forceinline__ int64_t whpd_first(const u64 *__restrict__ k, int64_t S, u64 key) {
  int64_t lo = 0, hi = S - 1;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (k[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the first j in [i, S) with C[j] >= need, or -1 where C[S - 1] < need
static __device__ __forceinline__ int64_t whpd_end(const u64 *__restrict__ C, int64_t S, int64_t i, u64 need) {
  if (C[S - 1] < need) return -1;
  int64_t lo = i, hi = S - 1;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (C[mid] < need) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// C[rl S + first position of sample s's key] += q[s], C zeroed before; workgroup (256 samples, rl).  Integer atomics:
// exact in any order
__global__ __launch_bounds__(256) void whpd_place_kernel(const double *V, int64_t row_stride, int64_t elem_stride, int64_t S,
                                                         int64_t row0, int64_t nblk, const u64 *__restrict__ sorted,
                                                         const u64 *__restrict__ q, u64 *__restrict__ C) {
  const int64_t rl = blockIdx.x / nblk, s = (blockIdx.x % nblk) * 256 + threadIdx.x;
  if (s >= S) return;
  const u64 wt = q[s];
  if (wt == 0) return;
  const u64 key = rk_key(V[(row0 + rl) * row_stride + s * elem_stride]);
  atomicAdd(&C[rl * S + whpd_first(sorted + rl * S, S, key)], wt);
}

// cs[rl nsc + c] = the sum of chunk c of WH_SCAN positions of C; workgroup (c, rl)
__global__ __launch_bounds__(256) void whpd_chunksum_kernel(const u64 *__restrict__ C, int64_t S, int64_t nsc,
                                                            u64 *__restrict__ cs) {
  __shared__ u64 red[256];
  const int64_t c = blockIdx.x % nsc, rl = blockIdx.x / nsc;
  u64 a = 0;
  for (int j = 0; j < WH_SCAN / 256; ++j) {
    const int64_t i = c * WH_SCAN + (int64_t)threadIdx.x * (WH_SCAN / 256) + j;
    if (i < S) a += C[rl * S + i];
  }
  a = wg_sum_a<256>(a, red);
  if (threadIdx.x == 0) cs[blockIdx.x] = a;
}

// cs[rl nsc + .] becomes its exclusive prefix sum; one workgroup per row: thread t owns a contiguous piece
__global__ __launch_bounds__(256) void whpd_chunkscan_kernel(u64 *__restrict__ cs, int64_t nsc) {
  __shared__ u64 piece[256];
  const int tid = threadIdx.x;
  u64 *p = cs + (int64_t)blockIdx.x * nsc;
  const int64_t per = (nsc + 255) / 256, c0 = (int64_t)tid * per, c1 = (c0 + per < nsc) ? c0 + per : nsc;
  u64 a = 0;
  for (int64_t c = c0; c < c1; ++c) a += p[c];
  piece[tid] = a;
  __syncthreads();
  if (tid == 0) {
    u64 run = 0;
    for (int t = 0; t < 256; ++t) {
      const u64 v = piece[t];
      piece[t] = run;
      run += v;
    }
  }
  __syncthreads();
  u64 run = piece[tid];
  for (int64_t c = c0; c < c1; ++c) {
    const u64 v = p[c];
    p[c] = run;
    run += v;
  }
}

// C becomes its inclusive prefix sum along the row, chunk c starting from cs[rl nsc + c]; workgroup (c, rl)
__global__ __launch_bounds__(256) void whpd_apply_kernel(u64 *__restrict__ C, int64_t S, int64_t nsc,
                                                         const u64 *__restrict__ cs) {
  __shared__ u64 tsum[256];
  constexpr int PER = WH_SCAN / 256;
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x % nsc, rl = blockIdx.x / nsc, i0 = c * WH_SCAN + (int64_t)tid * PER;
  u64 v[PER], a = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    v[j] = (i0 + j < S) ? C[rl * S + i0 + j] : 0;
    a += v[j];
  }
  tsum[tid] = a;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {   // inclusive scan of the threads' sums
    const u64 add = tid >= off ? tsum[tid - off] : 0;
    __syncthreads();
    tsum[tid] += add;
    __syncthreads();
  }
  u64 run = cs[blockIdx.x] + tsum[tid] - a;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    run += v[j];
    if (i0 + j < S) C[rl * S + i0 + j] = run;
  }
}

// pw / pi[(rl L + l) nchunk + c] = the minimum of (k[j(i)] - k[i], i) over the run starts i of chunk c that have an end
__global__ __launch_bounds__(256) void whpd_window_kernel(const u64 *__restrict__ sorted, const u64 *__restrict__ C,
                                                          int64_t S, int n_levels, const u64 *__restrict__ targets,
                                                          int64_t nchunk, double *__restrict__ pw,
                                                          long long *__restrict__ pi) {
  __shared__ double sw[256];
  __shared__ long long si[256];
  const int64_t c = blockIdx.x % nchunk, rl_l = blockIdx.x / nchunk, rl = rl_l / n_levels;
  const u64 t = targets[rl_l % n_levels];
  const u64 *k = sorted + rl * S, *cw = C + rl * S;
  double bw = INFINITY;
  long long bi = 0x7fffffffffffffffll;
  for (int j = 0; j < HW_PER / 256; ++j) {
    const int64_t i = c * HW_PER + (int64_t)j * 256 + threadIdx.x;
    if (i < S && (i == 0 || k[i] != k[i - 1])) {
      const int64_t e = whpd_end(cw, S, i, (i ? cw[i - 1] : (u64)0) + t);
      if (e >= 0) {
        const double w = sel_value(k[e]) - sel_value(k[i]);
        if (hpd_before(w, i, bw, bi)) { bw = w; bi = i; }
      }
    }
  }
  hpd_wg_min(bw, bi, sw, si);
  if (threadIdx.x == 0) {
    pw[blockIdx.x] = bw;
    pi[blockIdx.x] = bi;
  }
}

// out[((pair0 + rl) L + l) 2 + {0, 1}] = the two ends; workgroup (rl, l)
__global__ __launch_bounds__(256) void whpd_finish_kernel(const u64 *__restrict__ sorted, const u64 *__restrict__ C,
                                                          int64_t S, int n_levels, const u64 *__restrict__ targets,
                                                          int64_t nchunk, const double *__restrict__ pw,
                                                          const long long *__restrict__ pi, const int *__restrict__ nan,
                                                          int64_t pair0, double *__restrict__ out) {
  __shared__ double sw[256];
  __shared__ long long si[256];
  const int64_t rl = blockIdx.x / n_levels;
  double bw = INFINITY;
  long long bi = 0x7fffffffffffffffll;
  for (int64_t c = threadIdx.x; c < nchunk; c += 256) {
    const double w = pw[(int64_t)blockIdx.x * nchunk + c];
    const long long i = pi[(int64_t)blockIdx.x * nchunk + c];
    if (hpd_before(w, i, bw, bi)) { bw = w; bi = i; }
  }
  hpd_wg_min(bw, bi, sw, si);
  if (threadIdx.x == 0) {
    const u64 *k = sorted + rl * S, *cw = C + rl * S;
    const double smin = sel_value(k[0]), smax = sel_value(k[S - 1]);
    double lo = sel_nan(), hi = lo;
    // (the sentinel index survives where no run start has an end -- t exceeds Q -- and where every width is a NaN)
    if (!nan[rl] && !isinf(smin) && !isinf(smax) && bi >= 0 && bi < S) {
      const int64_t e = whpd_end(cw, S, bi, (bi ? cw[bi - 1] : (u64)0) + targets[blockIdx.x % n_levels]);
      if (e >= 0) {
        lo = sel_value(k[bi]);
        hi = sel_value(k[e]);
      }
    }
    double *o = out + ((pair0 + rl) * n_levels + blockIdx.x % n_levels) * 2;
    o[0] = lo;
    o[1] = hi;
  }
}

static int whpd_check(int64_t R_v, int64_t S, int64_t R_w, int64_t n_levels, const u64 *targets) {
  GP_ARG(R_v > 0, "R_v must be positive");
  GP_ARG(R_w >= 1 && R_w <= WS_MAX_RW, "R_w must be in [1, 64]");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(R_v <= ((1ll << 31) - 1) / R_w, "R_v * R_w must be below 2^31");
  GP_ARG(n_levels > 0 && n_levels <= 4096 && targets, "n_levels must be in [1, 4096]");
  for (int64_t i = 0; i < R_w * n_levels; ++i)
    GP_ARG(targets[i] >= 1 && targets[i] <= (1ull << 53), "every target must be in [1, 2^53]");
  return GPEMU_OK;
}

// bytes of workspace of one (weight row, value row) pair of a batch: the sort's, the cumulative weights, the chunk sums of
// the prefix sum, the windows' (pw, pi)
static inline int64_t whpd_pair_bytes(int64_t S, int64_t n_levels) {
  return rank_row_bytes(S) + 8 * S + 8 * ((S + WH_SCAN - 1) / WH_SCAN) + 16 * n_levels * ((S + HW_PER - 1) / HW_PER);
}

// the intervals of R_v value rows under R_w weight rows: the value rows in batches that fit workspace_bytes, sorted once
// for all weight rows; waits for st
static int whpd_rows(const double *dV, int64_t R_v, int64_t S, int64_t row_stride, int64_t elem_stride, int64_t R_w,
                     const u64 *dq, int64_t ldq, int64_t n_levels, const u64 *targets, double *dout,
                     int64_t workspace_bytes, hipStream_t st) {
  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t nchunk = (S + HW_PER - 1) / HW_PER, nsc = (S + WH_SCAN - 1) / WH_SCAN, nblk = (S + 255) / 256;
  const int64_t per_pair = whpd_pair_bytes(S, n_levels);
  const int64_t rows_cap = sort_rows_cap(R_v, S, budget, per_pair, n_levels * nchunk);
  if (rows_cap < 1) {
    set_error("weighted_hpd: out of memory: one (weight row, value row) pair of %lld elements and %lld levels needs %lld "
              "bytes of sort, prefix-sum and window buffers; %lld bytes %s", (long long)S, (long long)n_levels,
              (long long)per_pair, (long long)budget, workspace_budget_name(workspace_bytes));
    return GPEMU_ERR_HIP;
  }
  DevScope sc(st);
  SortScratch sort;
  u64 *dt = nullptr, *C = nullptr, *cs = nullptr;
  double *pw = nullptr;
  long long *pi = nullptr;
  GP_TRY(sort.alloc(sc, rows_cap, S));
  GP_TRY(sc.alloc(&dt, R_w * n_levels));
  GP_TRY(sc.alloc(&C, rows_cap * S));
  GP_TRY(sc.alloc(&cs, rows_cap * nsc));
  GP_TRY(sc.alloc(&pw, rows_cap * n_levels * nchunk));
  GP_TRY(sc.alloc(&pi, rows_cap * n_levels * nchunk));
  GP_TRY(upload(dt, targets, R_w * n_levels, st));
  for (int64_t row0 = 0; row0 < R_v; row0 += rows_cap) {
    const int64_t rows = std::min(rows_cap, R_v - row0);
    wsummary_path_count(GPEMU_WSUMMARY_PATH_HPD_SORT_BATCH);
    GP_TRY(sort_rows(dV, row_stride, elem_stride, S, row0, rows, sort, [] {}, st));
    for (int64_t w = 0; w < R_w; ++w) {
      GP_HIP(hipMemsetAsync(C, 0, sizeof(u64) * (size_t)(rows * S), st));
      wsummary_path_count(GPEMU_WSUMMARY_PATH_HPD_PLACE);
      hipLaunchKernelGGL(whpd_place_kernel, dim3((unsigned)(rows * nblk)), dim3(256), 0, st, dV, row_stride, elem_stride, S,
                         row0, nblk, (const u64 *)sort.ka, dq + w * ldq, C);
      GP_HIP(hipGetLastError());
      wsummary_path_count(GPEMU_WSUMMARY_PATH_HPD_SCAN);
      hipLaunchKernelGGL(whpd_chunksum_kernel, dim3((unsigned)(rows * nsc)), dim3(256), 0, st, (const u64 *)C, S, nsc, cs);
      hipLaunchKernelGGL(whpd_chunkscan_kernel, dim3((unsigned)rows), dim3(256), 0, st, cs, nsc);
      hipLaunchKernelGGL(whpd_apply_kernel, dim3((unsigned)(rows * nsc)), dim3(256), 0, st, C, S, nsc, (const u64 *)cs);
      GP_HIP(hipGetLastError());
      wsummary_path_count(GPEMU_WSUMMARY_PATH_HPD_WINDOW);
      hipLaunchKernelGGL(whpd_window_kernel, dim3((unsigned)(rows * n_levels * nchunk)), dim3(256), 0, st,
                         (const u64 *)sort.ka, (const u64 *)C, S, (int)n_levels, (const u64 *)(dt + w * n_levels), nchunk,
                         pw, pi);
      GP_HIP(hipGetLastError());
      hipLaunchKernelGGL(whpd_finish_kernel, dim3((unsigned)(rows * n_levels)), dim3(256), 0, st, (const u64 *)sort.ka,
                         (const u64 *)C, S, (int)n_levels, (const u64 *)(dt + w * n_levels), nchunk, (const double *)pw,
                         (const long long *)pi, (const int *)sort.nan, w * R_v + row0, dout);
      GP_HIP(hipGetLastError());
    }
  }
  GP_HIP(hipStreamSynchronize(st));   // the targets are read by the copy above
  return GPEMU_OK;
}

// ---- kernel density ------------------------------------------------------------------------------------------------
// part[((rl G) + g) nchunk + c] = sum over the samples j of chunk c of exp(-((grid[r][g] - x_rj) inv_h[r])^2 / 2);
// workgroup (c, tile, rl).  Wt: the weights of the samples
struct KdeUnit {   // none: every sample counts 1 (gpemu_kde1d)
  static constexpr bool weighted = false;
};
struct KdeFixed {  // fixed-point weights (gpemu_weighted_kde1d): row r is the pair (w, v) = (r / R_v, r % R_v) of
  static constexpr bool weighted = true;   // weight row w and value row v, and the term of sample j is (double)q_wj exp(.)
  const u64 *q;                            // [R_w][ldq]
  int64_t ldq, R_v;
};
template <int GPT, class Wt>
__global__ __launch_bounds__(256) void kde_partial_kernel(const double *__restrict__ V, int64_t row_stride,
                                                          int64_t elem_stride, int64_t S, int64_t row0,
                                                          const double *__restrict__ grid,
                                                          const double *__restrict__ inv_h, int64_t G, int64_t nchunk,
                                                          double *__restrict__ part, Wt wt) {
  __shared__ double xs[Wt::weighted ? 2 * KD_STAGE : KD_STAGE];   // the samples, then their weights
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x, rl = blockIdx.z, r = row0 + rl;
  const double ih = inv_h[r];
  const double *x = V + r * row_stride;
  const u64 *qrow = nullptr;
  if constexpr (Wt::weighted) {
    x = V + (r % wt.R_v) * row_stride;
    qrow = wt.q + (r / wt.R_v) * wt.ldq;
  }
  double g[GPT], acc[GPT][4];
#pragma unroll
  for (int k = 0; k < GPT; ++k) {
    const int64_t gi = ((int64_t)blockIdx.y * GPT + k) * 256 + tid;
    g[k] = gi < G ? grid[r * G + gi] : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[k][q] = 0.0;
  }
  const int64_t j0 = c * KD_CHUNK, j1 = (j0 + KD_CHUNK < S) ? j0 + KD_CHUNK : S;
  for (int64_t s0 = j0; s0 < j1; s0 += KD_STAGE) {
    const int n = (int)((j1 - s0 < KD_STAGE) ? j1 - s0 : KD_STAGE);
    __syncthreads();
    for (int t = tid; t < n; t += 256) {
      xs[t] = x[(s0 + t) * elem_stride];
      if constexpr (Wt::weighted) xs[KD_STAGE + t] = (double)qrow[s0 + t];   // exact: q < 2^53
    }
    __syncthreads();
    for (int t = 0; t < n; t += 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (t + q < n) {
          const double xv = xs[t + q];
          if constexpr (Wt::weighted) {
            const double qd = xs[KD_STAGE + t + q];
            if (qd != 0.0) {   // a sample of weight 0 contributes nothing
#pragma unroll
              for (int k = 0; k < GPT; ++k) {
                const double u = (g[k] - xv) * ih;
                const double e = -0.5 * (u * u);
                if (e > -746.0) acc[k][q] = fma(qd, exp(e), acc[k][q]);
              }
            }
          } else {
#pragma unroll
            for (int k = 0; k < GPT; ++k) {
              const double u = (g[k] - xv) * ih;
              const double e = -0.5 * (u * u);
              if (e > -746.0) acc[k][q] += exp(e);   // below: exactly 0 in fp64
            }
          }
        }
    }
  }
#pragma unroll
  for (int k = 0; k < GPT; ++k) {
    const int64_t gi = ((int64_t)blockIdx.y * GPT + k) * 256 + tid;
    if (gi < G) part[(rl * G + gi) * nchunk + c] = (acc[k][0] + acc[k][1]) + (acc[k][2] + acc[k][3]);
  }
}

// dens[(row0 + rl) G + g] = norm[row0 + rl] * the sum of the grid point's chunk sums; workgroup (rl, g)
__global__ __launch_bounds__(256) void kde_sum_kernel(const double *__restrict__ part, int64_t nchunk, int64_t G,
                                                      int64_t row0, const double *__restrict__ norm,
                                                      double *__restrict__ dens) {
  __shared__ double ws[4];
  const int tid = threadIdx.x;
  const double *p = part + (int64_t)blockIdx.x * nchunk;
  double a = 0.0;
  for (int64_t c = tid; c < nchunk; c += 256) a += p[c];
  a = wg_sum_b<4>(a, ws);
  if (tid == 0) {
    const int64_t rl = blockIdx.x / G, g = blockIdx.x % G;
    dens[(row0 + rl) * G + g] = a * norm[row0 + rl];
  }
}

static int kde_check(int64_t R, int64_t S, int64_t G, const double *grid, const double *h) {
  GP_ARG(R > 0 && S > 0 && G > 0, "R, S and G must be positive");
  GP_ARG(grid && h, "null pointer");
  GP_ARG(R <= ((1ll << 31) - 1) / G, "R * G must be below 2^31");
  for (int64_t r = 0; r < R; ++r) GP_ARG(std::isfinite(h[r]) && h[r] > 0.0, "every bandwidth must be finite and > 0");
  for (int64_t i = 0; i < R * G; ++i) GP_ARG(std::isfinite(grid[i]), "grid points must be finite");
  return GPEMU_OK;
}

// the densities of R rows (Wt = KdeFixed: of R pairs); total[r]: what row r's sum is divided by, S or Q_w
template <class Wt>
static int kde_rows(const double *dV, int64_t R, int64_t S, int64_t row_stride, int64_t elem_stride, int64_t G,
                    const double *grid, const double *h, const double *total, double *ddens, Wt wt, hipStream_t st) {
  const int64_t nchunk = (S + KD_CHUNK - 1) / KD_CHUNK;
  const int gpt = G <= 256 ? 1 : (G <= 512 ? 2 : KD_MAX_GPT);
  const int64_t ntile = (G + 256 * gpt - 1) / (256 * gpt);
  GP_ARG(ntile <= 65535, "G must be at most 65535 * 1024");
  int64_t rows_cap = std::max<int64_t>(1, KD_PART_BYTES / (8 * G * nchunk));
  rows_cap = std::min<int64_t>(std::min<int64_t>(rows_cap, R), 65535);
  rows_cap = std::min<int64_t>(rows_cap, std::max<int64_t>(1, (int64_t)0x7fffffff / G));
  std::vector<double> ih((size_t)R), norm((size_t)R);
  for (int64_t r = 0; r < R; ++r) {
    ih[(size_t)r] = 1.0 / h[r];
    norm[(size_t)r] = 1.0 / (total[r] * h[r] * std::sqrt(2.0 * M_PI));
  }
  DevScope sc(st);
  double *dgrid = nullptr, *dih = nullptr, *dnorm = nullptr, *part = nullptr;
  GP_TRY(sc.alloc(&dgrid, R * G));
  GP_TRY(sc.alloc(&dih, R));
  GP_TRY(sc.alloc(&dnorm, R));
  GP_TRY(sc.alloc(&part, rows_cap * G * nchunk));
  GP_TRY(upload(dgrid, grid, R * G, st));
  GP_TRY(upload(dih, ih.data(), R, st));
  GP_TRY(upload(dnorm, norm.data(), R, st));
  for (int64_t row0 = 0; row0 < R; row0 += rows_cap) {
    const int64_t rows = std::min(rows_cap, R - row0);
    if (Wt::weighted)
      wsummary_path_count(GPEMU_WSUMMARY_PATH_KDE);
    else
      marginal_path_count(GPEMU_MARGINAL_PATH_KDE);
    const dim3 gr((unsigned)nchunk, (unsigned)ntile, (unsigned)rows);
    if (gpt == 1)
      hipLaunchKernelGGL((kde_partial_kernel<1, Wt>), gr, dim3(256), 0, st, dV, row_stride, elem_stride, S, row0, dgrid, dih,
                         G, nchunk, part, wt);
    else if (gpt == 2)
      hipLaunchKernelGGL((kde_partial_kernel<2, Wt>), gr, dim3(256), 0, st, dV, row_stride, elem_stride, S, row0, dgrid, dih,
                         G, nchunk, part, wt);
    else
      hipLaunchKernelGGL((kde_partial_kernel<KD_MAX_GPT, Wt>), gr, dim3(256), 0, st, dV, row_stride, elem_stride, S, row0,
                         dgrid, dih, G, nchunk, part, wt);
    hipLaunchKernelGGL(kde_sum_kernel, dim3((unsigned)(rows * G)), dim3(256), 0, st, part, nchunk, G, row0, dnorm, ddens);
    GP_HIP(hipGetLastError());
  }
  GP_HIP(hipStreamSynchronize(st));   // ih and norm are read by the copies above
  return GPEMU_OK;
}

static int wkde_check(int64_t R_v, int64_t S, int64_t R_w, int64_t G, const double *grid, const double *h) {
  GP_ARG(R_v > 0, "R_v must be positive");
  GP_ARG(R_w >= 1 && R_w <= WS_MAX_RW, "R_w must be in [1, 64]");
  GP_ARG(S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(R_v <= ((1ll << 31) - 1) / R_w, "R_v * R_w must be below 2^31");
  return kde_check(R_w * R_v, S, G, grid, h);
}

// the densities of the R_w R_v pairs under the weights dq: Q_w read back first, then kde_rows over the pairs; waits for st
static int wkde_rows(const double *dV, int64_t R_v, int64_t S, int64_t row_stride, int64_t elem_stride, int64_t R_w,
                     const u64 *dq, int64_t ldq, int64_t G, const double *grid, const double *h, double *ddens,
                     hipStream_t st) {
  std::vector<u64> Q((size_t)R_w);
  {
    DevScope sc(st);
    u64 *dQ = nullptr;
    GP_TRY(sc.alloc(&dQ, R_w));
    GP_TRY(weight_totals(dq, ldq, R_w, S, dQ, st));
    GP_TRY(sc.download(Q.data(), dQ, R_w));
    GP_HIP(hipStreamSynchronize(st));
  }
  std::vector<double> total((size_t)(R_w * R_v));
  for (int64_t r = 0; r < R_w * R_v; ++r) total[(size_t)r] = (double)Q[(size_t)(r / R_v)];
  return kde_rows(dV, R_w * R_v, S, row_stride, elem_stride, G, grid, h, total.data(), ddens, KdeFixed{dq, ldq, R_v}, st);
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_marginal_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_MARGINAL, out, n); }

int gpemu_marginal_hist_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows,
                            int64_t block_stride_rows, int d, int nb1, const double *edges1, int nb2,
                            const double *edges2, int64_t group_counters, int64_t *dhist1, int64_t *dhist2,
                            int64_t *dn_inside1, void *stream) {
  GP_ARG(dX, "null pointer");
  RowsView X;
  GP_TRY(rows_view(dX, n_blocks, block_rows, block_stride_rows, d, &X));
  GP_TRY(hist_check(d, nb1, edges1, nb2, edges2, group_counters, dhist1, dhist2, dn_inside1));
  GP_TRY(device_ready(device));
  return count_rows(X, nb1, edges1, nb2, edges2, group_counters, dhist1, dhist2, dn_inside1, (hipStream_t)stream);
}

int gpemu_marginal_hist(int device, int64_t S, int d, const double *X, int nb1, const double *edges1, int nb2,
                        const double *edges2, int64_t group_counters, int64_t *hist1, int64_t *hist2,
                        int64_t *n_inside1) {
  GP_ARG(X, "null pointer");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_TRY(hist_check(d, nb1, edges1, nb2, edges2, group_counters, hist1, hist2, n_inside1));
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  const int64_t np = d * (d - 1) / 2, n2 = np * nb2 * nb2;
  DevScope sc(st);
  double *dX = nullptr;
  int64_t *dh1 = nullptr, *dh2 = nullptr, *dni = nullptr;
  GP_TRY(sc.alloc(&dX, S * d));
  GP_TRY(sc.alloc(&dh1, (int64_t)d * nb1));
  GP_TRY(sc.alloc(&dh2, n2));
  GP_TRY(sc.alloc(&dni, d));
  GP_TRY(upload(dX, X, S * d, st));
  GP_TRY(count_rows(RowsView{dX, 1, S, S * d, d}, nb1, edges1, nb2, edges2, group_counters, dh1, dh2, dni, st));
  GP_TRY(sc.download(hist1, dh1, (int64_t)d * nb1));
  if (n2 > 0) GP_TRY(sc.download(hist2, dh2, n2));
  GP_TRY(sc.download(n_inside1, dni, d));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_hpd_dev(int device, int64_t R, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                  int64_t n_levels, const int64_t *n_out, double *dout, int64_t workspace_bytes, void *stream) {
  GP_ARG(dV && dout, "null pointer");
  GP_TRY(hpd_check(R, S, n_levels, n_out));
  GP_ARG(row_stride > 0 && elem_stride > 0, "strides must be positive");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  GP_TRY(device_ready(device));
  return hpd_rows(dV, R, S, row_stride, elem_stride, n_levels, n_out, dout, workspace_bytes, (hipStream_t)stream);
}

int gpemu_hpd(int device, int64_t R, int64_t S, const double *V, int64_t n_levels, const int64_t *n_out, double *out) {
  GP_ARG(V && out, "null pointer");
  GP_TRY(hpd_check(R, S, n_levels, n_out));
  GP_ARG(R <= INT64_MAX / 8 / S, "R * S overflows");
  return with_host_rows(device, R, S, V, n_levels * 2, out, [&](const double *dV, double *dout, hipStream_t st) {
    return hpd_rows(dV, R, S, S, 1, n_levels, n_out, dout, 0, st);
  });
}

int gpemu_kde1d_dev(int device, int64_t R, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                    int64_t G, const double *grid, const double *h, double *ddens, void *stream) {
  GP_ARG(dV && ddens, "null pointer");
  GP_TRY(kde_check(R, S, G, grid, h));
  GP_ARG(row_stride > 0 && elem_stride > 0, "strides must be positive");
  GP_TRY(device_ready(device));
  const std::vector<double> total((size_t)R, (double)S);
  return kde_rows(dV, R, S, row_stride, elem_stride, G, grid, h, total.data(), ddens, KdeUnit{}, (hipStream_t)stream);
}

int gpemu_kde1d(int device, int64_t R, int64_t S, const double *V, int64_t G, const double *grid, const double *h,
                double *dens) {
  GP_ARG(V && dens, "null pointer");
  GP_TRY(kde_check(R, S, G, grid, h));
  GP_ARG(R <= INT64_MAX / 8 / S, "R * S overflows");
  const std::vector<double> total((size_t)R, (double)S);
  return with_host_rows(device, R, S, V, G, dens, [&](const double *dV, double *dd, hipStream_t st) {
    return kde_rows(dV, R, S, S, 1, G, grid, h, total.data(), dd, KdeUnit{}, st);
  });
}

int gpemu_weighted_hpd_dev(int device, int64_t R_v, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                           int64_t R_w, const uint64_t *dq, int64_t ldq, int64_t n_levels, const uint64_t *targets,
                           double *dout, const gpemu_call_ctx *ctx) {
  GP_ARG(dV && dq && dout, "null pointer");
  GP_TRY(whpd_check(R_v, S, R_w, n_levels, (const u64 *)targets));
  GP_ARG(row_stride > 0 && elem_stride > 0, "strides must be positive");
  GP_ARG(ldq >= S, "ldq must be at least S");
  GP_ARG(ctx_workspace(ctx) >= 0, "workspace_bytes must be >= 0");
  GP_TRY(device_ready(device));
  return whpd_rows(dV, R_v, S, row_stride, elem_stride, R_w, (const u64 *)dq, ldq, n_levels, (const u64 *)targets, dout,
                   ctx_workspace(ctx), ctx_stream(ctx));
}

int gpemu_weighted_hpd(int device, int64_t R_v, int64_t S, const double *V, int64_t R_w, const uint64_t *q,
                       int64_t n_levels, const uint64_t *targets, double *out) {
  GP_ARG(V && q && out, "null pointer");
  GP_TRY(whpd_check(R_v, S, R_w, n_levels, (const u64 *)targets));
  GP_ARG(R_v <= INT64_MAX / 8 / S, "R_v * S overflows");
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  DevScope sc(st);
  double *dV = nullptr, *dout = nullptr;
  u64 *dq = nullptr;
  GP_TRY(sc.alloc(&dV, R_v * S));
  GP_TRY(sc.alloc(&dq, R_w * S));
  GP_TRY(sc.alloc(&dout, R_w * R_v * n_levels * 2));
  GP_TRY(upload(dV, V, R_v * S, st));
  GP_TRY(upload(dq, (const u64 *)q, R_w * S, st));
  GP_TRY(whpd_rows(dV, R_v, S, S, 1, R_w, dq, S, n_levels, (const u64 *)targets, dout, 0, st));
  GP_TRY(sc.download(out, dout, R_w * R_v * n_levels * 2));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_weighted_kde1d_dev(int device, int64_t R_v, int64_t S, const double *dV, int64_t row_stride,
                             int64_t elem_stride, int64_t R_w, const uint64_t *dq, int64_t ldq, int64_t G,
                             const double *grid, const double *h, double *ddens, const gpemu_call_ctx *ctx) {
  GP_ARG(dV && dq && ddens, "null pointer");
  GP_TRY(wkde_check(R_v, S, R_w, G, grid, h));
  GP_ARG(row_stride > 0 && elem_stride > 0, "strides must be positive");
  GP_ARG(ldq >= S, "ldq must be at least S");
  GP_TRY(device_ready(device));
  return wkde_rows(dV, R_v, S, row_stride, elem_stride, R_w, (const u64 *)dq, ldq, G, grid, h, ddens, ctx_stream(ctx));
}

int gpemu_weighted_kde1d(int device, int64_t R_v, int64_t S, const double *V, int64_t R_w, const uint64_t *q, int64_t G,
                         const double *grid, const double *h, double *dens) {
  GP_ARG(V && q && dens, "null pointer");
  GP_TRY(wkde_check(R_v, S, R_w, G, grid, h));
  GP_ARG(R_v <= INT64_MAX / 8 / S, "R_v * S overflows");
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  DevScope sc(st);
  double *dV = nullptr, *dd = nullptr;
  u64 *dq = nullptr;
  GP_TRY(sc.alloc(&dV, R_v * S));
  GP_TRY(sc.alloc(&dq, R_w * S));
  GP_TRY(sc.alloc(&dd, R_w * R_v * G));
  GP_TRY(upload(dV, V, R_v * S, st));
  GP_TRY(upload(dq, (const u64 *)q, R_w * S, st));
  GP_TRY(wkde_rows(dV, R_v, S, S, 1, R_w, dq, S, G, grid, h, dd, st));
  GP_TRY(sc.download(dens, dd, R_w * R_v * G));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_marginal_dense_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows,
                             int64_t block_stride_rows, int d, double *ddense, void *stream) {
  GP_ARG(dX && ddense, "null pointer");
  RowsView X;
  GP_TRY(rows_view(dX, n_blocks, block_rows, block_stride_rows, d, &X));
  GP_TRY(device_ready(device));
  hipStream_t st = (hipStream_t)stream;
  GP_TRY(gather_rows(X, 0, X.rows(), ddense, st));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_marginal_moments_dev(int device, const double *dX, int64_t S, int d, double *mean, double *var, void *stream) {
  GP_ARG(dX && mean && var, "null pointer");
  GP_ARG(S > 0 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(d >= 1 && d <= ROWS_MAX_D, "d must be in [1, 16]");
  GP_TRY(device_ready(device));
  return moments_to_host(dX, S, d, mean, var, (hipStream_t)stream);
}

}  // extern "C"
