// What the summaries of a stored chain share.  k_rows.hip: the view of a chain as blocks of rows
// with its checks and its gather, the pooled moments, the workspace budget, the key-only radix sort of rows with its
// scratch; here, the host form of a function of device rows.  k_select.hip: the radix select, counted and weighted.
// k_marginal.hip: the histogram sweep, counted and weighted.  k_wsummary.hip: the weighted row sums, and
// here what a gpemu_call_ctx says.  The summaries' own kernels -- window search, density,
// split, rank lookup, log-ratios -- stay in their files.
#pragma once
#include <algorithm>

#include "internal.h"
#include "sampler_internal.h"

namespace gpemu {

// ---- rows in blocks ------------------------------------------------------------------------------------------------
// n_blocks blocks of block_rows rows of d doubles; block b starts block_stride ELEMENTS after block b - 1 (a stride in
// elements: a step of a chain may be padded to a length that is no multiple of d).  Logical row r is row r % block_rows
// of block r / block_rows: the sampler's chain in place, thinned by steps, one chain of a stacked sampler.
struct RowsView {
  const double *base;
  int64_t n_blocks, block_rows, block_stride;
  int d;
  __host__ __device__ int64_t rows() const { return n_blocks * block_rows; }
  __host__ __device__ const double *row(int64_t r) const {
    return base + (r / block_rows) * block_stride + (r % block_rows) * d;
  }
  bool dense() const { return n_blocks == 1 || block_stride == block_rows * d; }
};
// GPEMU_ERR_ARG unless the blocks are non-empty and do not overlap; the callers add their own limits
int rows_check(const RowsView &v);
// the rows of a summary's _dev call (a stride in ROWS) as a view, within the summaries' limits: d <= ROWS_MAX_D, fewer
// than 2^31 rows
constexpr int ROWS_MAX_D = 16;
int rows_view(const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows, int d, RowsView *v);
// dst[n][d] = logical rows [r0, r0 + n) of v; asynchronous on st
int gather_rows(const RowsView &v, int64_t r0, int64_t n, double *dst, hipStream_t st);

// ---- pooled moments ------------------------------------------------------------------------------------------------
// dmom[0 .. d) = mean, dmom[d .. 2d) = variance (divisor R) of the R rows of dx [R][d], two passes with sums in a fixed
// order (thread t its rows t, t + 256, ... of a block of MOM_ROWS, then tree A of wg_dev.h; the block partials the same
// way); dpart: (R + MOM_ROWS - 1) / MOM_ROWS * d doubles of scratch; asynchronous on st
constexpr int MOM_ROWS = 1024;
int launch_moments(const double *dx, int64_t R, int d, double *dpart, double *dmom, hipStream_t st);
// the final stage alone: dout[e] = (the sum over the nb blocks of dpart[b][e]) / R, e < nent; the caller checks the
// launch
void launch_moments_final(const double *dpart, int64_t nb, int nent, int64_t R, double *dout, hipStream_t st);
// ... with its scratch, into host mean [d] and var [d]; waits for st
int moments_to_host(const double *dx, int64_t R, int d, double *mean, double *var, hipStream_t st);

// the pooled mean alone of a view of rows of any width (k_kde2d.hip: pm_partial_kernel, then the final stage above);
// dpart: (rows + MOM_ROWS - 1) / MOM_ROWS * d doubles of scratch; asynchronous on st
int launch_pooled_mean(const RowsView &v, double *dpart, double *dmean, hipStream_t st);

// ---- workspace budget ----------------------------------------------------------------------------------------------
// *budget = workspace_bytes, or half of the free memory of the current device where that is 0
int workspace_budget(int64_t workspace_bytes, int64_t *budget);
// how an out-of-memory message names that budget, after "%lld bytes "
const char *workspace_budget_name(int64_t workspace_bytes);

// ---- key-only LSD radix sort of rows of doubles (the kernels' comments: k_rows.hip) ----------------------------------
constexpr int RK_PASSES = 8;       // 8 bits each
constexpr int RK_BINS = 256;
constexpr int RK_TILE = 2048;      // keys per workgroup: 4 waves x 8 rounds x 64 lanes

static __device__ __forceinline__ u64 rk_key(double v) {
  if (v == 0.0) v = 0.0;   // -0 and +0 are tied
  return sel_key(v);
}

// bytes of the sort's buffers for one row of S elements: two key arrays, the (digit, tile) histogram, the NaN flag
static inline int64_t rank_row_bytes(int64_t S) { return 16 * S + 4 * RK_BINS * ((S + RK_TILE - 1) / RK_TILE) + 4; }
// rows of S elements per batch: what budget holds at per_row bytes each, at most R, and no more than a flattened grid
// of (rows, 256-element blocks) -- or of (rows, grid_per_row workgroups) -- can address.  Below 1: out of memory
int64_t sort_rows_cap(int64_t R, int64_t S, int64_t budget, int64_t per_row, int64_t grid_per_row = 1);

struct SortScratch {
  u64 *ka = nullptr, *kb = nullptr;   // [rows_cap][S] keys; the sorted keys end in ka
  unsigned *hist = nullptr;           // [rows_cap][RK_BINS][tiles]
  int *nan = nullptr;                 // [rows_cap] the row holds a NaN
  int alloc(DevScope &sc, int64_t rows_cap, int64_t S);
};
// sorts the keys of `rows` rows from row0 on (elements dV[row row_stride + i elem_stride], i < S) into s.ka; s.nan[rl] = 1
// for a row that holds a NaN.  on_pass() is called once per pass (path counters).  Asynchronous on st
int sort_rows(const double *dV, int64_t row_stride, int64_t elem_stride, int64_t S, int64_t row0, int64_t rows,
              const SortScratch &s, void (*on_pass)(), hipStream_t st);

// ---- radix select of rows of doubles, by count or by weight (k_select.hip) ------------------------------
constexpr int SEL_BINS = 256;      // 8 bits a pass
constexpr int SEL_MAXT = 16;       // targets (and slots) per group
constexpr int SEL_ROWS = 512;      // (weight row, value row) pairs per batch, at most: 16 MiB of global histograms
constexpr int64_t SEL_ROW_BYTES = 8ll * SEL_MAXT * SEL_BINS + 3 * 8 * SEL_MAXT + 2 * 4 * SEL_MAXT + 8;   // state of one pair
// dout[(w R_v + v) nt_all + i] = the smallest element x of value row v (elements dV[v row_stride + s elem_stride], s < S)
// with sum_{x_s <= x} q[w][s] >= targets[w nt_all + i], NaN where the row holds a NaN or no element answers.  dq null:
// every weight is 1 (R_w = 1), so target t is the order statistic of rank t - 1.  targets: on the host, each >= 1.  The
// pairs go through the state in batches of rows_cap <= SEL_ROWS, the caller's choice (SEL_ROW_BYTES each); on_pass() is
// called once per pass of a batch and a group of targets (path counters).  Waits for st
int select_rows(const double *dV, int64_t R_v, int64_t S, int64_t row_stride, int64_t elem_stride, int64_t R_w,
                const u64 *dq, int64_t ldq, int64_t nt_all, const u64 *targets, double *dout, int64_t rows_cap,
                void (*on_pass)(), hipStream_t st);

// ---- histogram sweep over a view of rows, by count or by weight (k_marginal.hip) ------------------------
constexpr int64_t HIST_CAP16 = 73728;   // 16-bit counters of a counted sweep: 144 KiB of LDS
constexpr int64_t HIST_CAP64 = 18432;   // 64-bit bins of a weighted sweep: 144 KiB of LDS
// GPEMU_ERR_ARG unless the d rows of nb + 1 edges are finite and strictly increasing
int edges_check(const double *e, int d, int nb);
// dhist1[w][d][nb1], dhist2[w][np][nb2][nb2] = the sums of q[w][s] (dq null: of 1, R_w = 1) over the rows s of X in each
// bin of the host edges; dinside1[w][j] = the sum of dhist1[w][j][.].  cap: bins of one sweep, at most HIST_CAP64
// (HIST_CAP16 without weights), at least max(nb1, nb2) (max(nb1, nb2^2)).  on_sweep(pairs) is called once per sweep,
// pairs: it holds 2-D bins (path counters).  Waits for st
int hist_rows(const RowsView &X, int64_t R_w, const u64 *dq, int64_t ldq, int nb1, const double *edges1, int nb2,
              const double *edges2, int64_t cap, u64 *dhist1, u64 *dhist2, u64 *dinside1, void (*on_sweep)(bool pairs),
              hipStream_t st);

// ---- weighted row reductions under fixed-point weights (k_wsummary.hip) ---------------------------------
constexpr int64_t WS_SUM = 4096;   // samples per partial sum: the chunks of k_postpred.hip's tree
constexpr int WS_MAX_RW = 64;      // weight rows per call of the weighted summaries
// what a gpemu_call_ctx says: null is stream NULL, workspace_bytes 0
static inline hipStream_t ctx_stream(const gpemu_call_ctx *ctx) { return ctx ? (hipStream_t)ctx->stream : nullptr; }
static inline int64_t ctx_workspace(const gpemu_call_ctx *ctx) { return ctx ? ctx->workspace_bytes : 0; }
// dQ[w] = the integer sum of dq[w][0 .. S); asynchronous on st
int weight_totals(const u64 *dq, int64_t ldq, int64_t R_w, int64_t S, u64 *dQ, hipStream_t st);
// out[w ldo + r] = sum_s q_ws x_rs / Q_w (centre null) or sum_s q_ws (x_rs - centre[w ldc + r])^2 / Q_w for the R rows
// x_rs = X[r rs + s es], in the tree fixed by the sample index.  part: R_w ldp ceil(S / WS_SUM) doubles of scratch,
// ldp >= R.  Asynchronous on st
int weighted_rowmean(const double *X, int64_t rs, int64_t es, int64_t R, int64_t S, int64_t R_w, const u64 *dq,
                     int64_t ldq, const u64 *dQ, const double *centre, int64_t ldc, double *part, int64_t ldp,
                     double *out, int64_t ldo, hipStream_t st);

// ---- the host form of a function of device rows --------------------------------------------------------------------
// device_ready, V [R][S] to the device, fn(dV, dout, stream) on rows of strides (S, 1), dout [R][out_per_row] back, wait
template <class Fn>
static int with_host_rows(int device, int64_t R, int64_t S, const double *V, int64_t out_per_row, double *out, Fn &&fn) {
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  DevScope sc(st);
  double *dV = nullptr, *dout = nullptr;
  GP_TRY(sc.alloc(&dV, R * S));
  GP_TRY(sc.alloc(&dout, R * out_per_row));
  GP_TRY(upload(dV, V, R * S, st));
  GP_TRY(fn(dV, dout, st));
  GP_TRY(sc.download(out, dout, R * out_per_row));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

}  // namespace gpemu
