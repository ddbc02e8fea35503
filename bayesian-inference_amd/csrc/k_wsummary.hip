// Weighted row reductions for the summaries of a reweighted chain (gpemu_posterior_predictive_weighted*):
// the weighted mean and the weighted centred second moment of many rows under many rows of fixed-point weights at once.
//
//   ws_total_kernel   Q[w] = the integer sum of weight row w (tree A on integers, one 64-bit global integer atomic per
//                     workgroup: exact in any order);
//   ws_rowsum_kernel  workgroup (chunk c of WS_SUM = 4096 samples, WS_FT rows, WS_WR weight rows): the x of its rows and
//                     the q of its weight rows are loaded once and shared by the WS_FT x WS_WR sums
//                       part[(w ldp + row) nchunk + c] = sum over the chunk of (double)q_ws x_s          (centre null)
//                                                     or of ((double)q_ws (x_s - centre[w][row])) (x_s - centre[w][row])
//                     in the tree of pp_rowsum_kernel (k_postpred.hip): a lane adds its 16 terms in index order -- one
//                     fused multiply-add each, a term of weight 0 left out -- then tree B of wg_dev.h;
//   ws_finish_kernel  out[w][row] = (the chunk sums added in chunk order) / (double)Q[w].
// Every q and every Q is below 2^53, so (double)q and (double)Q are exact.  A sum depends on the values and on that tree
// alone: not on how rows and weight rows are grouped into workgroups or launches, on the workspace or on the run.  With
// q_s = 2^e the sums are 2^e times pp_rowsum_kernel's, bit for bit.  No floating-point atomics.
#include <algorithm>

#include "internal.h"
#include "rows_dev.h"
#include "sampler_internal.h"
#include "wg_dev.h"

namespace gpemu {

constexpr int WS_FT = 4;   // rows per workgroup
constexpr int WS_WR = 4;   // weight rows per workgroup

__global__ __launch_bounds__(256) void ws_total_kernel(const u64 *__restrict__ q, int64_t ldq, int64_t S,
                                                       u64 *__restrict__ Q) {
  __shared__ u64 red[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  const u64 s = wg_sum_a<256>(i < S ? q[w * ldq + i] : (u64)0, red);
  if (threadIdx.x == 0 && s) atomicAdd(&Q[w], s);
}

struct WsArgs {
  const double *X;         // row r, element i: X[r rs + i es]
  int64_t rs, es, S, R;
  const u64 *q;            // [R_w][ldq]
  int64_t ldq, R_w;
  const double *centre;    // [R_w][ldc] or null
  int64_t ldc;
  double *part;            // [R_w][ldp][nchunk]
  int64_t ldp, nchunk;
};

__global__ __launch_bounds__(256) void ws_rowsum_kernel(WsArgs a) {
  __shared__ double ws[4];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x, r0 = (int64_t)blockIdx.y * WS_FT, w0 = (int64_t)blockIdx.z * WS_WR;
  // a row or a weight row past the end repeats the last one: loaded, never stored
  const double *x[WS_FT];
  const u64 *q[WS_WR];
  double mu[WS_FT][WS_WR], acc[WS_FT][WS_WR];
#pragma unroll
  for (int f = 0; f < WS_FT; ++f) x[f] = a.X + ((r0 + f < a.R) ? r0 + f : a.R - 1) * a.rs;
#pragma unroll
  for (int r = 0; r < WS_WR; ++r) q[r] = a.q + ((w0 + r < a.R_w) ? w0 + r : a.R_w - 1) * a.ldq;
#pragma unroll
  for (int f = 0; f < WS_FT; ++f)
#pragma unroll
    for (int r = 0; r < WS_WR; ++r) {
      acc[f][r] = 0.0;
      mu[f][r] = (a.centre && r0 + f < a.R && w0 + r < a.R_w) ? a.centre[(w0 + r) * a.ldc + r0 + f] : 0.0;
    }
  for (int j = 0; j < WS_SUM / 256; ++j) {
    const int64_t i = c * WS_SUM + (int64_t)j * 256 + tid;
    if (i < a.S) {
      double xv[WS_FT], qd[WS_WR];
#pragma unroll
      for (int f = 0; f < WS_FT; ++f) xv[f] = x[f][i * a.es];
#pragma unroll
      for (int r = 0; r < WS_WR; ++r) qd[r] = (double)q[r][i];
#pragma unroll
      for (int f = 0; f < WS_FT; ++f)
#pragma unroll
        for (int r = 0; r < WS_WR; ++r) {
          const double dv = xv[f] - mu[f][r];
          const double t = a.centre ? fma(qd[r] * dv, dv, acc[f][r]) : fma(qd[r], xv[f], acc[f][r]);
          acc[f][r] = qd[r] != 0.0 ? t : acc[f][r];
        }
    }
  }
#pragma unroll
  for (int f = 0; f < WS_FT; ++f)
#pragma unroll
    for (int r = 0; r < WS_WR; ++r) {
      const double s = wg_sum_b<4>(acc[f][r], ws);
      if (tid == 0 && r0 + f < a.R && w0 + r < a.R_w) a.part[((w0 + r) * a.ldp + r0 + f) * a.nchunk + c] = s;
    }
}

// out[w ldo + row] = (sum of part[(w ldp + row) nchunk + .], in chunk order) / (double)Q[w]; thread (row, w)
__global__ __launch_bounds__(256) void ws_finish_kernel(const double *__restrict__ part, int64_t ldp, int64_t nchunk,
                                                        int64_t R, const u64 *__restrict__ Q, double *__restrict__ out,
                                                        int64_t ldo) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (row >= R) return;
  const double *p = part + (w * ldp + row) * nchunk;
  double acc = 0.0;
  for (int64_t c = 0; c < nchunk; ++c) acc += p[c];
  out[w * ldo + row] = acc / (double)Q[w];
}

int weight_totals(const u64 *dq, int64_t ldq, int64_t R_w, int64_t S, u64 *dQ, hipStream_t st) {
  GP_HIP(hipMemsetAsync(dQ, 0, sizeof(u64) * (size_t)R_w, st));
  hipLaunchKernelGGL(ws_total_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)R_w), dim3(256), 0, st, dq, ldq, S, dQ);
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

int weighted_rowmean(const double *X, int64_t rs, int64_t es, int64_t R, int64_t S, int64_t R_w, const u64 *dq,
                     int64_t ldq, const u64 *dQ, const double *centre, int64_t ldc, double *part, int64_t ldp,
                     double *out, int64_t ldo, hipStream_t st) {
  WsArgs a;
  a.X = X; a.rs = rs; a.es = es; a.S = S; a.q = dq; a.ldq = ldq; a.R_w = R_w;
  a.centre = centre; a.ldc = ldc; a.part = part; a.ldp = ldp; a.nchunk = (S + WS_SUM - 1) / WS_SUM;
  const unsigned gz = (unsigned)((R_w + WS_WR - 1) / WS_WR);
  for (int64_t r0 = 0; r0 < R; r0 += 32768 * WS_FT) {   // grid.y
    const int64_t nr = std::min<int64_t>(32768 * WS_FT, R - r0);
    a.X = X + r0 * rs; a.R = nr;
    a.centre = centre ? centre + r0 : nullptr;
    a.part = part + r0 * a.nchunk;
    wsummary_path_count(GPEMU_WSUMMARY_PATH_ROW_REDUCE);
    hipLaunchKernelGGL(ws_rowsum_kernel, dim3((unsigned)a.nchunk, (unsigned)((nr + WS_FT - 1) / WS_FT), gz), dim3(256), 0,
                       st, a);
    GP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(ws_finish_kernel, dim3((unsigned)((R + 255) / 256), (unsigned)R_w), dim3(256), 0, st,
                     (const double *)part, ldp, a.nchunk, R, dQ, out, ldo);
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_wsummary_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_WSUMMARY, out, n); }

}  // extern "C"
