// k-th nearest-neighbour distances of chain rows in the unit box (gpemu_unit_rows_dev, gpemu_knn_dist*,
// gpemu_knn_logsum_dev): what the Kozachenko-Leonenko entropy and the Wang-Kulkarni-Verdu / Perez-Cruz
// divergence estimators need of a chain -- the information gain the reference leaves open (ref: plot_qhat.py:116,
// plot_analyses.py:144).
//
// unit_rows_kernel: U[i] = ((x - lo) * inv_width of logical row floor(i S / n) of the view), two separately rounded
// operations per coordinate; a row with a non-finite coordinate becomes a row of NaN and is counted.
//
// knn_search_kernel<DP, CAP>: workgroup (256 queries, subset, reference split).  A thread owns one query: its DP
// coordinates of the subset and a sorted list of the CAP smallest squared distances so far, all in statically indexed
// registers.  The references of the split stream through LDS KNN_TILE at a time, the subset's columns only, one array
// per column: every lane reads the same address (a broadcast).  Per pair: acc = fma(diff, diff, acc) over the subset's
// coordinates in increasing order, then ONE compare with the current k-th distance; the rare taken branch tells a copy
// (acc == 0: counted, not a neighbour) from a neighbour (inserted).  The references are taken 4, 2 or 1 at a time by
// DP, so that their LDS reads are in flight together; the compares keep the references' order.  The list holds
// CAP - k sentinels of -inf in front, so that the k-th smallest is always a[CAP - 1] whatever k is: no dynamic index,
// nothing in scratch.  A subset of fewer than DP coordinates is padded with coordinates that are 0 in query and
// reference: fma(0, 0, acc) = acc.
// A reference with a non-finite coordinate gives inf or NaN and is never below the k-th distance; a query with one
// gets r2 = NaN.  knn_merge_kernel<CAP>: the k smallest of the Z partial lists of a query, and the sum of its Z zero
// counts.  The k smallest of a set do not depend on the order of the set: the bits are the same for every Z and tile.
//
// knn_logsum_*: per subset the counts and the sums of log r2 (or of log nu2 - log rho2) and of its square over blocks
// of LS_ROWS rows, each by tree A of wg_dev.h; then the blocks' partials by tree A.  No floating-point atomics.
#include <algorithm>
#include <cmath>
#include <vector>

#include "internal.h"
#include "rows_dev.h"
#include "wg_dev.h"

namespace gpemu {

constexpr int KNN_MAX_D = 16;
constexpr int KNN_TILE = GPEMU_KNN_REF_TILE;   // references in LDS at a time: one per thread
constexpr int KNN_MAX_SPLITS = 64;
constexpr int KNN_MIN_SPLIT = 64;              // the fewest references a split is chosen to hold
constexpr int KNN_TARGET_WGS = 2048;           // workgroups a launch should have before it stops splitting
constexpr int LS_ROWS = 1024;                  // rows per partial of the log sums
static_assert(KNN_TILE == 256, "a thread stages one reference of the tile");

static inline void knn_path_count(int path) { count_path(PATHS_KNN, path); }   // enum gpemu_knn_path

// ---- unit-box rows ---------------------------------------------------------------------------------------------------
struct UnitBox {
  double lo[KNN_MAX_D], iw[KNN_MAX_D];
};

__global__ __launch_bounds__(256) void unit_rows_kernel(RowsView v, UnitBox box, int64_t n, double *__restrict__ U,
                                                        unsigned long long *__restrict__ skipped) {
#pragma clang fp contract(off)   // the subtraction and the product round on their own: numpy's bits
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int d = v.d;
  const double *row = v.row(i * v.rows() / n);   // i S < 2^62
  bool ok = true;
  for (int j = 0; j < d; ++j) ok = ok && isfinite(row[j]);
  for (int j = 0; j < d; ++j) {
    const double t = row[j] - box.lo[j];
    U[i * d + j] = ok ? t * box.iw[j] : __builtin_nan("");
  }
  if (!ok) atomicAdd(skipped, 1ull);   // an integer count: its value does not depend on the order
}

// ---- the search --------------------------------------------------------------------------------------------------------
// the CAP smallest values seen, ascending; a[0 .. CAP - k) are sentinels that never move, a[CAP - 1] is the k-th
template <int CAP>
struct TopK {
  double a[CAP];
  __device__ __forceinline__ void init(int k) {
#pragma unroll
    for (int j = 0; j < CAP; ++j) a[j] = j < CAP - k ? -INFINITY : INFINITY;
  }
  __device__ __forceinline__ double kth() const { return a[CAP - 1]; }
  // x < kth(), x is no NaN: the largest goes, every slot takes the middle one of its left neighbour, itself and x
  __device__ __forceinline__ void insert(double x) {
#pragma unroll
    for (int j = CAP - 1; j > 0; --j) {
      const double lo = a[j - 1], me = a[j];
      a[j] = lo > x ? lo : (me > x ? x : me);
    }
    a[0] = a[0] > x ? x : a[0];
  }
};

struct KnnArgs {
  const double *UQ, *UR;   // [nq][d], [nr][d]
  int64_t nq, nr, chunk;   // chunk: references per split
  int d, k, Z, np;         // np: subsets of this launch
  const int *order;        // [np] the subset of blockIdx.y
  const int *cols;         // [P][KNN_MAX_D] the subset's coordinates, increasing, then -1
  double *r2;              // [P][nq]           (Z == 1: written here)
  int *zeros;              // [P][nq]
  double *part;            // [Z][np][k][nq]    (Z > 1)
  int *pzeros;             // [Z][np][nq]
};

template <int DP, int CAP>
__global__ __launch_bounds__(256) void knn_search_kernel(KnnArgs g) {
  __shared__ double sR[DP * KNN_TILE];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const int y = blockIdx.y, z = blockIdx.z;
  const int p = g.order[y];
  int c[DP];
#pragma unroll
  for (int j = 0; j < DP; ++j) c[j] = g.cols[p * KNN_MAX_D + j];
  const bool live = i < g.nq;
  bool ok = true;
  double q[DP];
#pragma unroll
  for (int j = 0; j < DP; ++j) {
    q[j] = (live && c[j] >= 0) ? g.UQ[i * g.d + c[j]] : 0.0;
    ok = ok && isfinite(q[j]);
  }
  TopK<CAP> top;
  top.init(g.k);
  int zeros = 0;
  const int64_t r0 = (int64_t)z * g.chunk, r1 = (r0 + g.chunk < g.nr) ? r0 + g.chunk : g.nr;
  for (int64_t t0 = r0; t0 < r1; t0 += KNN_TILE) {
    const int n = (int)((r1 - t0 < KNN_TILE) ? r1 - t0 : KNN_TILE);
    __syncthreads();   // the previous tile has been read
    if (tid < n) {
#pragma unroll
      for (int j = 0; j < DP; ++j) sR[j * KNN_TILE + tid] = c[j] >= 0 ? g.UR[(t0 + tid) * g.d + c[j]] : 0.0;
    }
    __syncthreads();
    if (live && ok) {
      // G references at a time: their LDS reads are issued together and their chains run side by side, then the
      // compares in the references' order -- the same operations per pair, the same order of insertions
      constexpr int G = DP <= 4 ? 4 : (DP <= 8 ? 2 : 1);
      int t = 0;
      for (; t + G <= n; t += G) {
        double acc[G];
#pragma unroll
        for (int u = 0; u < G; ++u) acc[u] = 0.0;
#pragma unroll
        for (int j = 0; j < DP; ++j) {
#pragma unroll
          for (int u = 0; u < G; ++u) {
            const double diff = q[j] - sR[j * KNN_TILE + t + u];
            acc[u] = fma(diff, diff, acc[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
          if (acc[u] < top.kth()) {   // the k-th distance is > 0: a copy passes this test too
            if (acc[u] == 0.0) ++zeros;
            else top.insert(acc[u]);
          }
        }
      }
      for (; t < n; ++t) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < DP; ++j) {
          const double diff = q[j] - sR[j * KNN_TILE + t];
          acc = fma(diff, diff, acc);
        }
        if (acc < top.kth()) {
          if (acc == 0.0) ++zeros;
          else top.insert(acc);
        }
      }
    }
  }
  if (!live) return;
  if (g.Z == 1) {
    g.r2[(int64_t)p * g.nq + i] = ok ? top.kth() : __builtin_nan("");
    g.zeros[(int64_t)p * g.nq + i] = zeros;
    return;
  }
  const int64_t zy = (int64_t)z * g.np + y;
#pragma unroll
  for (int j = 0; j < CAP; ++j)
    if (j >= CAP - g.k) g.part[(zy * g.k + (j - (CAP - g.k))) * g.nq + i] = ok ? top.a[j] : __builtin_nan("");
  g.pzeros[zy * g.nq + i] = zeros;
}

// thread (query, subset of the launch): the k smallest of its Z lists; a NaN in them marks a query that is passed over
template <int CAP>
__global__ __launch_bounds__(256) void knn_merge_kernel(KnnArgs g) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.nq) return;
  const int y = blockIdx.y, p = g.order[y];
  TopK<CAP> top;
  top.init(g.k);
  int zeros = 0;
  bool bad = false;
  for (int z = 0; z < g.Z; ++z) {
    const int64_t zy = (int64_t)z * g.np + y;
    for (int j = 0; j < g.k; ++j) {
      const double x = g.part[(zy * g.k + j) * g.nq + i];
      if (x != x) bad = true;
      else if (x < top.kth()) top.insert(x);
    }
    zeros += g.pzeros[zy * g.nq + i];
  }
  g.r2[(int64_t)p * g.nq + i] = bad ? __builtin_nan("") : top.kth();
  g.zeros[(int64_t)p * g.nq + i] = zeros;
}

// ---- the sums (tree A of wg_dev.h) ---------------------------------------------------------------------------------
// workgroup (block of LS_ROWS rows, subset): cnt[(p nb + b) 3 + .] = used, short, copies; sum[(p nb + b) 2 + .] = the
// sum of v and of v^2 over the used rows, v = log r2 or log nu2 - log r2.  A row is used if every distance is finite,
// short if none is NaN and one is +inf; a NaN distance passes it over.
__global__ __launch_bounds__(256) void knn_logsum_partial_kernel(int64_t n, const double *__restrict__ r2,
                                                                 const int *__restrict__ zeros,
                                                                 const double *__restrict__ nu2,
                                                                 long long *__restrict__ cnt, double *__restrict__ sum) {
  __shared__ double redd[256];
  __shared__ long long redi[256];
  const int t = threadIdx.x;
  const int64_t p = blockIdx.y, nb = gridDim.x, b = blockIdx.x;
  const int64_t i0 = b * LS_ROWS, i1 = (i0 + LS_ROWS < n) ? i0 + LS_ROWS : n;
  long long used = 0, shrt = 0, copies = 0;
  double s = 0.0, s2 = 0.0;
  for (int64_t i = i0 + t; i < i1; i += 256) {
    const double a = r2[p * n + i], c = nu2 ? nu2[p * n + i] : 1.0;
    if (zeros) copies += zeros[p * n + i];
    if (a != a || c != c) continue;
    if (isinf(a) || isinf(c)) {
      ++shrt;
      continue;
    }
    const double v = nu2 ? log(c) - log(a) : log(a);
    ++used;
    s += v;
    s2 = fma(v, v, s2);
  }
  used = wg_sum_a<256>(used, redi);
  shrt = wg_sum_a<256>(shrt, redi);
  copies = wg_sum_a<256>(copies, redi);
  s = wg_sum_a<256>(s, redd);
  s2 = wg_sum_a<256>(s2, redd);
  if (t == 0) {
    long long *pc = cnt + (p * nb + b) * 3;
    pc[0] = used; pc[1] = shrt; pc[2] = copies;
    sum[(p * nb + b) * 2] = s;
    sum[(p * nb + b) * 2 + 1] = s2;
  }
}

// workgroup p: the partials of its blocks, strided over the threads in block order, then the tree
__global__ __launch_bounds__(256) void knn_logsum_final_kernel(int64_t nb, const long long *__restrict__ cnt,
                                                               const double *__restrict__ sum,
                                                               long long *__restrict__ ocnt, double *__restrict__ osum) {
  __shared__ double redd[256];
  __shared__ long long redi[256];
  const int64_t p = blockIdx.x;
  long long c[3] = {0, 0, 0};
  double s[2] = {0.0, 0.0};
  for (int64_t b = threadIdx.x; b < nb; b += 256) {
    for (int e = 0; e < 3; ++e) c[e] += cnt[(p * nb + b) * 3 + e];
    for (int e = 0; e < 2; ++e) s[e] += sum[(p * nb + b) * 2 + e];
  }
  for (int e = 0; e < 3; ++e) {
    const long long v = wg_sum_a<256>(c[e], redi);
    if (threadIdx.x == 0) ocnt[p * 3 + e] = v;
  }
  for (int e = 0; e < 2; ++e) {
    const double v = wg_sum_a<256>(s[e], redd);
    if (threadIdx.x == 0) osum[p * 2 + e] = v;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static const int KNN_DP_CLASSES[] = {1, 2, 3, 4, 6, 8, 12, 16};   // the instantiated widths of a subset
constexpr int KNN_N_CLASSES = (int)(sizeof(KNN_DP_CLASSES) / sizeof(int));

template <int DP>
static void knn_launch_search(int cap, dim3 grid, hipStream_t st, const KnnArgs &a) {
  if (cap == 4) hipLaunchKernelGGL((knn_search_kernel<DP, 4>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((knn_search_kernel<DP, 16>), grid, dim3(256), 0, st, a);
}

static void knn_launch_search(int dp, int cap, dim3 grid, hipStream_t st, const KnnArgs &a) {
  switch (dp) {
    case 1: knn_launch_search<1>(cap, grid, st, a); break;
    case 2: knn_launch_search<2>(cap, grid, st, a); break;
    case 3: knn_launch_search<3>(cap, grid, st, a); break;
    case 4: knn_launch_search<4>(cap, grid, st, a); break;
    case 6: knn_launch_search<6>(cap, grid, st, a); break;
    case 8: knn_launch_search<8>(cap, grid, st, a); break;
    case 12: knn_launch_search<12>(cap, grid, st, a); break;
    default: knn_launch_search<16>(cap, grid, st, a); break;
  }
}

static int knn_check(int64_t nq, int64_t nr, int d, const void *UQ, int64_t P, const uint32_t *masks, int k, int splits,
                     int64_t workspace_bytes, const void *r2, const void *zeros) {
  GP_ARG(UQ && masks && r2 && zeros, "null pointer");
  GP_ARG(d >= 1 && d <= KNN_MAX_D, "d must be in [1, 16]");
  GP_ARG(k >= 1 && k <= GPEMU_KNN_MAX_K, "k must be in [1, 16]");
  GP_ARG(nq >= 1 && nq < (1ll << 31) && nr >= 1 && nr < (1ll << 31), "nq and nr must be in [1, 2^31)");
  GP_ARG(P >= 1 && P <= (1 << 20), "n_subsets must be in [1, 2^20]");
  GP_ARG(splits >= 0 && splits <= KNN_MAX_SPLITS, "splits must be in [0, 64]");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  for (int64_t p = 0; p < P; ++p) {
    GP_ARG(masks[p] != 0, "a subset must name a coordinate");
    GP_ARG((masks[p] >> d) == 0, "a subset names a coordinate outside [0, d)");
  }
  return GPEMU_OK;
}

// r2, zeros [P][nq] of device rows; waits for st
static int knn_rows(int64_t nq, int64_t nr, int d, const double *dUQ, const double *dUR, int64_t P, const uint32_t *masks,
                    int k, int splits, int64_t workspace_bytes, double *dr2, int *dzeros, hipStream_t st) {
  const int cap = k <= 4 ? 4 : 16;
  const int64_t qt = (nq + 255) / 256;
  // the subsets by the width they run at, in their own order within a width
  std::vector<int> cols((size_t)(P * KNN_MAX_D), -1), order;
  std::vector<int> start(KNN_N_CLASSES + 1, 0);
  order.reserve((size_t)P);
  for (int c = 0; c < KNN_N_CLASSES; ++c) {
    for (int64_t p = 0; p < P; ++p) {
      const int dp = __builtin_popcount(masks[p]);
      if (dp > KNN_DP_CLASSES[c] || (c > 0 && dp <= KNN_DP_CLASSES[c - 1])) continue;
      order.push_back((int)p);
      for (int j = 0, e = 0; j < d; ++j)
        if (masks[p] >> j & 1u) cols[(size_t)(p * KNN_MAX_D + e++)] = j;
    }
    start[(size_t)c + 1] = (int)order.size();
  }
  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  DevScope sc(st);
  int *dcols = nullptr, *dorder = nullptr, *pzeros = nullptr;
  double *part = nullptr;
  GP_TRY(sc.alloc(&dcols, P * KNN_MAX_D));
  GP_TRY(sc.alloc(&dorder, P));
  GP_TRY(upload(dcols, cols.data(), P * KNN_MAX_D, st));
  GP_TRY(upload(dorder, order.data(), P, st));
  // one Z and one batch size for the call: the partial lists are allocated once
  int Z[KNN_N_CLASSES];
  int64_t batch[KNN_N_CLASSES], part_rows = 0;   // part_rows: the most Z * subsets of a batch
  const int64_t per_list = (8ll * k + 4) * nq;   // bytes of one split's list and zero count of one subset
  for (int c = 0; c < KNN_N_CLASSES; ++c) {
    const int64_t np = start[(size_t)c + 1] - start[(size_t)c];
    Z[c] = 1;
    batch[c] = std::min<int64_t>(np, 65535);
    if (np == 0) continue;
    int64_t z = splits;
    if (z == 0) {
      z = (KNN_TARGET_WGS + qt * np - 1) / (qt * np);
      z = std::min<int64_t>(z, (nr + KNN_MIN_SPLIT - 1) / KNN_MIN_SPLIT);
      z = std::max<int64_t>(1, std::min<int64_t>(z, KNN_MAX_SPLITS));
      z = std::min(z, std::max<int64_t>(1, budget / per_list));   // what the workspace holds of one subset
    }
    if (z > 1) {
      const int64_t fit = budget / (per_list * z);
      if (fit < 1) {
        set_error("knn: out of memory: %lld partial lists of one subset (%lld queries, k = %d) need %lld bytes; %lld "
                  "bytes %s", (long long)z, (long long)nq, k, (long long)(per_list * z), (long long)budget,
                  workspace_budget_name(workspace_bytes));
        return GPEMU_ERR_HIP;
      }
      batch[c] = std::min(batch[c], fit);
      part_rows = std::max(part_rows, z * batch[c]);
    }
    Z[c] = (int)z;
  }
  if (part_rows > 0) {
    GP_TRY(sc.alloc(&part, part_rows * k * nq));
    GP_TRY(sc.alloc(&pzeros, part_rows * nq));
  }
  KnnArgs a;
  a.UQ = dUQ; a.UR = dUR; a.nq = nq; a.nr = nr; a.d = d; a.k = k; a.cols = dcols; a.r2 = dr2; a.zeros = dzeros;
  a.part = part; a.pzeros = pzeros;
  for (int c = 0; c < KNN_N_CLASSES; ++c) {
    a.Z = Z[c];
    a.chunk = (nr + a.Z - 1) / a.Z;
    for (int64_t b0 = start[(size_t)c]; b0 < start[(size_t)c + 1]; b0 += batch[c]) {
      a.np = (int)std::min<int64_t>(batch[c], start[(size_t)c + 1] - b0);
      a.order = dorder + b0;
      knn_path_count(GPEMU_KNN_PATH_SUBSET_BATCH);
      knn_path_count(GPEMU_KNN_PATH_SEARCH);
      knn_launch_search(KNN_DP_CLASSES[c], cap, dim3((unsigned)qt, (unsigned)a.np, (unsigned)a.Z), st, a);
      GP_HIP(hipGetLastError());
      if (a.Z > 1) {
        knn_path_count(GPEMU_KNN_PATH_MERGE);
        const dim3 grid((unsigned)qt, (unsigned)a.np);
        if (cap == 4) hipLaunchKernelGGL(knn_merge_kernel<4>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(knn_merge_kernel<16>, grid, dim3(256), 0, st, a);
        GP_HIP(hipGetLastError());
      }
    }
  }
  GP_HIP(hipStreamSynchronize(st));   // the host vectors are read by the copies above
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_knn_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_KNN, out, n); }

int gpemu_unit_rows_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride, int d,
                        const double *lower, const double *upper, int64_t n, double *dU, int64_t *n_skipped, void *stream) {
  GP_ARG(dX && lower && upper && dU && n_skipped, "null pointer");
  GP_ARG(d >= 1 && d <= KNN_MAX_D, "d must be in [1, 16]");
  RowsView X{dX, n_blocks, block_rows, block_stride, d};
  GP_TRY(rows_check(X));
  GP_ARG(n_blocks <= ((1ll << 31) - 1) / block_rows, "S = n_blocks * block_rows must be in [1, 2^31)");
  GP_ARG(n >= 1 && n <= X.rows(), "n must be in [1, S]");
  UnitBox box;
  for (int j = 0; j < KNN_MAX_D; ++j) box.lo[j] = 0.0, box.iw[j] = 1.0;
  for (int j = 0; j < d; ++j) {
    GP_ARG(std::isfinite(lower[j]) && std::isfinite(upper[j]) && lower[j] < upper[j], "the box must be finite, lower < upper");
    box.lo[j] = lower[j];
    box.iw[j] = 1.0 / (upper[j] - lower[j]);
  }
  GP_TRY(device_ready(device));
  hipStream_t st = (hipStream_t)stream;
  DevScope sc(st);
  unsigned long long *dskip = nullptr, hskip = 0;
  GP_TRY(sc.alloc(&dskip, 1));
  GP_HIP(hipMemsetAsync(dskip, 0, sizeof(unsigned long long), st));
  knn_path_count(GPEMU_KNN_PATH_UNIT_ROWS);
  hipLaunchKernelGGL(unit_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, X, box, n, dU, dskip);
  GP_HIP(hipGetLastError());
  GP_TRY(sc.download(&hskip, dskip, 1));
  GP_HIP(hipStreamSynchronize(st));
  *n_skipped = (int64_t)hskip;
  return GPEMU_OK;
}

int gpemu_knn_dist_dev(int device, int64_t nq, int64_t nr, int d, const double *dUQ, const double *dUR, int64_t n_subsets,
                       const uint32_t *masks, int k, int splits, int64_t workspace_bytes, double *dr2, int32_t *dzeros,
                       void *stream) {
  GP_TRY(knn_check(nq, nr, d, dUQ, n_subsets, masks, k, splits, workspace_bytes, dr2, dzeros));
  GP_ARG(dUR || nr == nq, "a self search has nr = nq");
  GP_TRY(device_ready(device));
  return knn_rows(nq, nr, d, dUQ, dUR ? dUR : dUQ, n_subsets, masks, k, splits, workspace_bytes, dr2, dzeros,
                  (hipStream_t)stream);
}

int gpemu_knn_dist(int device, int64_t nq, int64_t nr, int d, const double *UQ, const double *UR, int64_t n_subsets,
                   const uint32_t *masks, int k, int splits, int64_t workspace_bytes, double *r2, int32_t *zeros) {
  GP_TRY(knn_check(nq, nr, d, UQ, n_subsets, masks, k, splits, workspace_bytes, r2, zeros));
  GP_ARG(UR || nr == nq, "a self search has nr = nq");
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  DevScope sc(st);
  double *dUQ = nullptr, *dUR = nullptr, *dr2 = nullptr;
  int *dzeros = nullptr;
  GP_TRY(sc.alloc(&dUQ, nq * d));
  GP_TRY(upload(dUQ, UQ, nq * d, st));
  if (UR) {
    GP_TRY(sc.alloc(&dUR, nr * d));
    GP_TRY(upload(dUR, UR, nr * d, st));
  }
  GP_TRY(sc.alloc(&dr2, n_subsets * nq));
  GP_TRY(sc.alloc(&dzeros, n_subsets * nq));
  GP_TRY(knn_rows(nq, nr, d, dUQ, UR ? dUR : dUQ, n_subsets, masks, k, splits, workspace_bytes, dr2, dzeros, st));
  GP_TRY(sc.download(r2, dr2, n_subsets * nq));
  GP_TRY(sc.download(zeros, dzeros, n_subsets * nq));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_knn_logsum_dev(int device, int64_t n_subsets, int64_t n, const double *dr2, const int32_t *dzeros,
                         const double *dnu2, int64_t *counts, double *sums, void *stream) {
  GP_ARG(dr2 && counts && sums, "null pointer");
  GP_ARG(n_subsets >= 1 && n_subsets <= 65535, "n_subsets must be in [1, 65535]");
  GP_ARG(n >= 1 && n < (1ll << 31), "n must be in [1, 2^31)");
  GP_TRY(device_ready(device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t P = n_subsets, nb = (n + LS_ROWS - 1) / LS_ROWS;
  DevScope sc(st);
  long long *cnt = nullptr, *ocnt = nullptr;
  double *sum = nullptr, *osum = nullptr;
  GP_TRY(sc.alloc(&cnt, P * nb * 3));
  GP_TRY(sc.alloc(&sum, P * nb * 2));
  GP_TRY(sc.alloc(&ocnt, P * 3));
  GP_TRY(sc.alloc(&osum, P * 2));
  knn_path_count(GPEMU_KNN_PATH_LOGSUM);
  hipLaunchKernelGGL(knn_logsum_partial_kernel, dim3((unsigned)nb, (unsigned)P), dim3(256), 0, st, n, dr2,
                     (const int *)dzeros, dnu2, cnt, sum);
  hipLaunchKernelGGL(knn_logsum_final_kernel, dim3((unsigned)P), dim3(256), 0, st, nb, (const long long *)cnt,
                     (const double *)sum, ocnt, osum);
  GP_HIP(hipGetLastError());
  static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as they are");
  GP_TRY(sc.download((long long *)counts, (const long long *)ocnt, P * 3));
  GP_TRY(sc.download(sums, (const double *)osum, P * 2));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

}  // extern "C"
