// GP predictive mean / variance for a batch of parameter points, all PCs of one emulation group.
//
// Replaces  ref: emulation.py:494-499  ->  skl _gpr.py:441-494  (GaussianProcessRegressor.predict
// with return_std=True, k times):
//     K_* = kernel_(X, X_train);  mean = K_* . alpha_;  V = L_^-1 K_*^T;  var = diag - sum_i V_i^2
// Device form: W = L_^-1 is formed once at model creation, so V = W K_*^T is a lower-triangular
// GEMM on the f64 matrix cores (v_mfma_f64_16x16x4_f64) with the column sum of squares fused into
// the epilogue -- V is never written to memory.
//
//   kstar_kernel          K_*^T[p][j][b] (HBM/L2 workspace) + partial means: the pairwise squared distance as a
//                         rank-8 product on the matrix cores (predict_dev.h), table exponential, HBM-write bound
//   trmm_vsq_dma_kernel   sum_i (W_p K_*^T)[i][b]^2 per 64-row block: persistent, LDS-direct loads, XCD-aware LPT
//                         schedule (MFMA f64); batches of at most 128 columns: k_trmm_small.hip
//   reduce_mean_var_kernel  sums the partials, var = kdiag - vsq, clip, std^2
#include <algorithm>

#include "internal.h"
#include "kstar_host.h"
#include "predict_dev.h"
#include "sched_host.h"

namespace gpemu {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------
// Cross-kernel.  grid (Bcap / 64, Npad / rows per workgroup, k), block 256 = 4 waves on a tile of
// WR JTW x 16 training rows x 64 queries (predict_dev.h: kstar_mfma_block).  The workgroup first puts its 64 raw query
// rows into LDS -- read from the padded buffer, padded on the fly from the caller's rows, or formed as the stretch
// proposal of the sampler -- two components per thread (four at the wide padding, DP = 16: d > 8).
struct KstarArgs {
  double *Xq;                          // [Bcap][DP] padded query rows (read, or written once per column block)
  const double *Xa, *alf, *qsc, *qof;  // matrix-core operands (kstar_host.h)
  const double *etab, *constv;
  const double *Xs, *inv_ls;           // Matern-0.5 / general nu < 1 only: row-major scaled training rows for the direct distance
  double *KS, *mean_part;
  int64_t N, Npad, Bcap;
  int has_const, d;
  int k, nchunk, ncb64;                // grid = ncb64 * nchunk * k workgroups (1-D)
  int gper, ncbp;                      // gper > 0: XCD-aware placement, gper of the k ncbp (PC, 128-column block) groups
                                       // of each piece of ncbp column blocks per XCD
  // the sampler's compacted half-step (internal.h: LiveCols): only the first ceil(*live / 64) column blocks hold queries,
  // and workgroup i of the grid's nwg takes the unit kmap[that count][i] (kstar_pack), or none (-1)
  const int *live, *kmap;
  int nwg;
};

// (the workgroup -> (PC, row chunk, 64-column block) unit of a whole batch, kstar_unit, and an entry of kmap, kstar_pack:
// sched_host.h)

// bidx: the workgroup's index within its group's grid; store_rows: this group's first workgroups keep the padded query
// rows / stretch factors (the first group of a launch that serves several: the others form the same rows and store nothing)
template <int KIND, int KS, int JTW, int NBW, int DP>
__device__ __forceinline__ void kstar_body(const KstarArgs &ka, const ProposeArgs &pa, const int bidx, const bool store_rows) {
  static_assert(DP == DPAD || DP == DPAD_WIDE, "padded width");
  constexpr int NC = DP / 4;                         // components of a query per thread
  __shared__ double s_tab[1 << KSTAR_TB];
  __shared__ __attribute__((aligned(16))) double s_q[64 * DP];
  __shared__ double s_red[4 * 64];
  constexpr int WC = 4 / NBW, WR = 4 / WC, JT = WR * JTW;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // Workgroups are dispatched round-robin over the 8 XCDs (workgroup i runs on XCD i % 8).  The triangular GEMM that
  // consumes K_*^T deals whole (PC, 128-column block) groups to XCDs (build_trmm_schedule: group g -> XCD g / gper), and
  // the L2s are kept coherent by hardware: a store to a line that ANOTHER XCD's L2 still holds from the GEMM's reads has
  // to invalidate it there first (measured: this kernel takes 13.5 us without the GEMM in between, 19.6 us behind it).
  // So each group's rows are written by the XCD that will read them: same L2, no cross-XCD traffic.
  int p, chunk, cb;
  const int nchunk = ka.nchunk;
  if (ka.live) {
    // compacted columns: the unit comes from the table of this launch's live block count (the same dealing as the
    // GEMM's schedule of that count), and a workgroup beyond its XCD's list has nothing to do
    const int c = (*ka.live + 63) >> 6;
    const int e = ka.kmap[(int64_t)(c < 0 ? 0 : (c > ka.ncb64 ? ka.ncb64 : c)) * ka.nwg + bidx];
    if (e < 0) return;
    p = e >> 20;
    chunk = (e >> 8) & 0xfff;
    cb = e & 0xff;
  } else {
    const KstarUnit u = kstar_unit(bidx, nchunk, ka.ncb64, ka.gper, ka.ncbp);
    p = u.p; chunk = u.chunk; cb = u.cb;
  }
  const int64_t b0 = (int64_t)cb * 64;
  const int64_t b = b0 + lane;
  // this thread's NC components of query b: wave, wave + 4, ...
  const int64_t njt = ka.Npad / 16;
  KstarFrags<KS, JTW> fr;
  if (threadIdx.x < (1 << KSTAR_TB)) s_tab[threadIdx.x] = ka.etab[threadIdx.x];
  const bool keeper = store_rows && chunk == 0 && p == 0;   // the workgroup that stores the padded rows of its columns
  double q[NC];
#pragma unroll
  for (int u = 0; u < NC; ++u) q[u] = 0.0;
  if (pa.enabled) {
    // stretch-move proposal for column b (every workgroup recomputes it; one of them stores it)
    if (b < pa.n) {
      const int w = pa.idx_s[b], j = pa.partner[b];
      const double z = pa.zz[b];
#pragma unroll
      for (int u = 0; u < NC; ++u) {
        const int c = wave + 4 * u;
        if (c < pa.d) {
          const double cj = pa.X[(int64_t)j * DP + c], sw = pa.X[(int64_t)w * DP + c];
          q[u] = cj - (cj - sw) * z;                 // emcee moves/stretch.py get_proposal
        }
      }
      if (keeper && wave == 0) pa.factors[b] = (pa.d - 1.0) * log(z);
    }
  } else if (pa.raw) {
    // caller rows [n][d]: padded on the fly
    if (b < pa.n) {
#pragma unroll
      for (int u = 0; u < NC; ++u)
        if (wave + 4 * u < pa.d) q[u] = pa.raw[b * pa.d + wave + 4 * u];
    }
  } else {
#pragma unroll
    for (int u = 0; u < NC; ++u) q[u] = ka.Xq[b * DP + wave + 4 * u];
  }
  if (keeper && (pa.enabled || pa.raw)) {
#pragma unroll
    for (int u = 0; u < NC; ++u) ka.Xq[b * DP + wave + 4 * u] = q[u];
  }
#pragma unroll
  for (int u = 0; u < NC; ++u) s_q[lane * DP + wave + 4 * u] = q[u];
  __syncthreads();
  // (requesting the fragments ahead of the proposal's loads was measured: 16.45 vs 16.1 us, slower)
  kstar_load_frags<KS, JTW, NBW>(fr, ka.Xa + (int64_t)p * njt * KS * 64, ka.alf + (int64_t)p * njt * 16, (int64_t)chunk * JT,
                                 lane, wave);
  const double c = ka.has_const ? ka.constv[p] : 0.0;
  KstarDirect dir{nullptr, nullptr};
  if (KIND == 1 || KIND == 4) dir = KstarDirect{ka.Xs + (int64_t)p * ka.Npad * DP, ka.inv_ls + p * DP};
  const MaternNu mn = (KIND == 4) ? kstar_matern_nu(ka.etab + (1 << KSTAR_TB)) : MaternNu();
  const double sum = kstar_mfma_block<KIND, KS, JTW, NBW, KSTAR_TB, 0, DP>(
      s_q, s_tab, s_red, fr, ka.qsc + p * 4 * KS, ka.qof + p * 4 * KS, c, ka.d, (int64_t)chunk * JT, ka.N, ka.KS + (int64_t)p * ka.Npad * ka.Bcap + b0, ka.Bcap, dir,
      lane, wave, mn);
  if (wave == 0) ka.mean_part[(b * ka.k + p) * nchunk + chunk] = sum;
}

template <int KIND, int KS, int JTW, int NBW, int DP>
__global__ __launch_bounds__(256, 2) void kstar_kernel(KstarArgs ka, ProposeArgs pa) {
  kstar_body<KIND, KS, JTW, NBW, DP>(ka, pa, (int)blockIdx.x, true);
}

// The cross-kernels of several emulation groups in ONE launch (a sampler over the shipped three groups spends its
// half-step in nine ~6 us launches otherwise): workgroups [start[g], start[g + 1]) are group g's grid.  Every group
// forms the stretch proposal itself (the same arithmetic, the same rows); the first one stores it.
constexpr int GROUPS_MAX = 8;
struct KstarGroups {
  KstarArgs g[GROUPS_MAX];
  int start[GROUPS_MAX + 1];
  int ng;
};
template <int KIND, int KS, int JTW, int NBW, int DP>
__global__ __launch_bounds__(256, 2) void kstar_groups_kernel(KstarGroups kg, ProposeArgs pa) {
  int gi = 0;
  while (gi + 1 < kg.ng && (int)blockIdx.x >= kg.start[gi + 1]) ++gi;
  kstar_body<KIND, KS, JTW, NBW, DP>(kg.g[gi], pa, (int)blockIdx.x - kg.start[gi], gi == 0);
}

// Columns per launch of the large-batch triangular GEMM.  More than 512 columns (emulation.predict on a large batch) go
// one launch per 512 columns: K_*^T of 1024 columns is 82 MB, and with W_p it no longer streams through the XCDs' L2s the
// way the 512-column schedule is built for (one launch of 1024 columns takes 228 us, two of 512 take 2 x 93 us).  Only
// when the pieces are equally wide (one cached schedule); else, and for stacked chains, the whole batch in one launch.
static int64_t trmm_piece_cols(const gpemu_model *m, int64_t B) {
  constexpr int64_t max_cols = 512;
  if (m->variant_B == 0 && B > max_cols) {
    const int64_t n = (B + max_cols - 1) / max_cols, per = round_up((B + n - 1) / n, TILE), last = B - (n - 1) * per;
    if (last > 0 && round_up(last, TILE) == per) return per;
  }
  return round_up(B, TILE);
}

// XCD whose workers will read rows (PC p, column col) of K_*^T in launch_trmm_vsq(m, B), or -1 if that launch places
// nothing XCD-aware: mirrors build_trmm_schedule / build_small_schedule (k_trmm_small.hip)
int trmm_xcd_of(const gpemu_model *m, int64_t B, int p, int64_t col) {
  const int64_t Bv = m->variant_B > 0 ? m->variant_B : B;
  if (Bv <= 128) return small_trmm_xcd_of(m, B, p, col);
  const int ncbp = (int)(trmm_piece_cols(m, B) / TILE), ngroups = (int)m->k * ncbp;
  if (ngroups % 8 != 0 || m->num_cu % 8 != 0) return -1;
  return (p * ncbp + (int)(col / TILE) % ncbp) / (ngroups / 8);
}

// which cross-kernel instance a launch takes (gpemu_path_counts)
static void kstar_count(const gpemu_model *m, bool small) {
  path_count(small ? GPEMU_PATH_KSTAR_SMALL : GPEMU_PATH_KSTAR_BIG);
  if (m->dp == DPAD) path_count(m->ksteps == 2 ? GPEMU_PATH_KSTAR_KSTEPS2 : GPEMU_PATH_KSTAR_KSTEPS3);
  else wide_path_count(m->ksteps == 3 ? GPEMU_WIDE_PATH_KSTAR_KSTEPS3 : m->ksteps == 4 ? GPEMU_WIDE_PATH_KSTAR_KSTEPS4
                                                                                        : GPEMU_WIDE_PATH_KSTAR_KSTEPS5);
  if (kstar_kind(m) == 1 || (kstar_kind(m) == 4 && m->nu < 1.0)) path_count(GPEMU_PATH_KSTAR_DIRECT);
}

// arguments and grid of one group's cross-kernel for a batch of B columns (sets the workspace's chunk count)
static KstarArgs kstar_setup(gpemu_model *m, int64_t B, double *dXq, int &nwg, bool &small) {
  // only the column tiles that hold real queries; without a proposal / raw rows, the rows of dXq up to
  // round_up(B, TILE) must be finite (the sampler's proposal buffer zeroes them)
  Workspace &w = m->ws;
  const int64_t Bv = m->variant_B > 0 ? m->variant_B : B;   // a chain stacked with others is evaluated as it would be alone
  small = Bv <= KSTAR_SMALL_MAX;                     // few columns: more, shorter workgroups
  const int rows_per_wg = small ? KSTAR_ROWS_SMALL : KSTAR_ROWS_BIG;
  w.cur_nchunk = (int)(m->Npad / rows_per_wg);
  // column blocks of 64 queries: whole 128-column tiles for the triangular GEMM, except that a batch of at most
  // 64 (always served by the small-batch kernel's 64-column items) needs only its first block
  const int64_t ncols = (B <= 64) ? 64 : round_up(B, TILE);
  const int ncb64 = (int)(ncols / 64);
  nwg = ncb64 * w.cur_nchunk * (int)m->k;
  // XCD-aware placement where the large-batch GEMM's schedule is (whole groups per XCD: build_trmm_schedule), piece by
  // piece of the columns as launch_trmm_vsq will cut them
  const int ncbp = (int)(trmm_piece_cols(m, B) / TILE);
  const int ngroups = (int)m->k * ncbp;
  const bool xcd_aware = Bv > 128 && ncb64 % 2 == 0 && (ncb64 / 2) % ncbp == 0 && ngroups % 8 == 0 && m->num_cu % 8 == 0;
  const int gper = xcd_aware ? ngroups / 8 : 0;
  return KstarArgs{dXq, m->Xa, m->alf, m->qsc, m->qof, m->etab, m->constv, m->Xs, m->inv_ls, w.KS, w.mean_part,
                   m->N, m->Npad, w.Bcap, m->has_const, (int)m->d, (int)m->k, w.cur_nchunk, ncb64, gper, ncbp,
                   nullptr, nullptr, nwg};
}

// instances: (ksteps, padded width) = (2, 8) d <= 7, (3, 8) d = 8; (3, 16) d = 9 .. 11, (4, 16) d = 12 .. 15, (5, 16) d = 16;
// JT = 1 for a small batch, else 2
#define GP_KSTAR_DISPATCH(KD, ksteps, dp, small, LAUNCH)                                                  \
  do {                                                                                                    \
    if ((dp) == DPAD) {                                                                                   \
      if ((ksteps) == 2) { if (small) LAUNCH(KD, 2, 1, DPAD); else LAUNCH(KD, 2, 2, DPAD); }              \
      else { if (small) LAUNCH(KD, 3, 1, DPAD); else LAUNCH(KD, 3, 2, DPAD); }                            \
    } else {                                                                                              \
      if ((ksteps) == 3) { if (small) LAUNCH(KD, 3, 1, DPAD_WIDE); else LAUNCH(KD, 3, 2, DPAD_WIDE); }    \
      else if ((ksteps) == 4) { if (small) LAUNCH(KD, 4, 1, DPAD_WIDE); else LAUNCH(KD, 4, 2, DPAD_WIDE); } \
      else { if (small) LAUNCH(KD, 5, 1, DPAD_WIDE); else LAUNCH(KD, 5, 2, DPAD_WIDE); }                  \
    }                                                                                                     \
  } while (0)

static int live_deal(gpemu_model *m, int ncb, int form, hipStream_t st, const gpemu_model::LiveDeal **out);

int launch_kstar(gpemu_model *m, int64_t B, double *dXq, hipStream_t st, const ProposeArgs *pa, const LiveCols *lv) {
  const ProposeArgs pargs = pa ? *pa : ProposeArgs();
  int nwg = 0;
  bool small = false;
  KstarArgs ka = kstar_setup(m, B, dXq, nwg, small);
  if (lv) {
    // compacted columns: the rows are in dXq already, and the workgroup -> unit map of the launch's live block count
    // comes from the table the GEMM's schedules are in (live_deal)
    const int ncb = (int)(round_up(B, TILE) / TILE);
    const gpemu_model::LiveDeal *deal = nullptr;
    GP_TRY(live_deal(m, ncb, lv->form, st, &deal));
    if (small || pargs.enabled || pargs.raw || ka.ncb64 != 2 * ncb || ka.ncbp != ncb || deal->nwg != nwg) {
      set_error("compacted columns: the cross-kernel takes them as one large-batch launch of rows it reads");
      return GPEMU_ERR_STATE;
    }
    ka.live = lv->n_live;
    ka.kmap = deal->kmap;
  }
  const dim3 grid((unsigned)nwg), block(256);
  const int pe0 = prof_mark(m, st);
#define GP_LAUNCH_ONE(KD, KSV, JT, DPV) hipLaunchKernelGGL((kstar_kernel<KD, KSV, JT, 2, DPV>), grid, block, 0, st, ka, pargs)
  GP_TRY(with_base_kind(kstar_kind(m), [&](auto kd) {
    GP_KSTAR_DISPATCH(decltype(kd)::value, m->ksteps, m->dp, small, GP_LAUNCH_ONE);
    return GPEMU_OK;
  }));
#undef GP_LAUNCH_ONE
  GP_HIP(hipGetLastError());
  kstar_count(m, small);
  prof_pair(m, 1, pe0, prof_mark(m, st));
  return GPEMU_OK;
}

// one launch for the cross-kernels of ng groups on the same B query rows (same base kernel and parameter count in all
// of them: the caller checks); `pa`: the stretch proposal, formed by every group, stored by the first
int launch_kstar_groups(gpemu_model *const *ms, int ng, int64_t B, double *dXq, hipStream_t st, const ProposeArgs *pa) {
  const ProposeArgs pargs = pa ? *pa : ProposeArgs();
  KstarGroups kg;
  kg.ng = ng;
  kg.start[0] = 0;
  bool small = false;
  for (int g = 0; g < ng; ++g) {
    int nwg = 0;
    kg.g[g] = kstar_setup(ms[g], B, dXq, nwg, small);
    kg.start[g + 1] = kg.start[g] + nwg;
  }
  const dim3 grid((unsigned)kg.start[ng]), block(256);
#define GP_LAUNCH_GROUPS(KD, KSV, JT, DPV) hipLaunchKernelGGL((kstar_groups_kernel<KD, KSV, JT, 2, DPV>), grid, block, 0, st, kg, pargs)
  GP_TRY(with_base_kind(kstar_kind(ms[0]), [&](auto kd) {
    GP_KSTAR_DISPATCH(decltype(kd)::value, ms[0]->ksteps, ms[0]->dp, small, GP_LAUNCH_GROUPS);
    return GPEMU_OK;
  }));
#undef GP_LAUNCH_GROUPS
  GP_HIP(hipGetLastError());
  kstar_count(ms[0], small);
  return GPEMU_OK;
}

// ------------------------------------------------------------------------------------------
// Triangular GEMM with fused column sum-of-squares.
//   V[i][b] = sum_{j<=i} Wt[j][i] * KS[j][b]      (per PC p; both operands are k-major)
//   out[b][p][rb] = sum_{i in 64-row block rb} V[i][b]^2
// MFMA v_mfma_f64_16x16x4_f64: lane l supplies A[i = l&15][k = l>>4], B[k = l>>4][n = l&15];
// D[reg] is row (l>>4) + 4*reg, column l&15 (verified by tools/mfma_f64_peak).
//
// One 512-thread workgroup per CU: 8 waves = 2 per SIMD, arranged 2 (M) x 4 (N), 32 x 32 per wave
// (2 x 2 MFMA tiles, 16 accumulator registers) on a 64 x 128 tile with K step 32.  Persistent: one workgroup per CU
// walks a host-built list of items (LPT schedule over the known K extents, so the triangular work is balanced to within
// one small item) as ONE software-pipelined stream of k-tiles.  Items of the first quarter of the rows (short K) are
// split into two 64-column halves to give the schedule small pieces for its tail.  Measured history (C3, B = 512):
// 128x128 tiles / 4 waves 182 us; 64x128 / 2 workgroups per CU 123 us; one item per workgroup, 8 waves 117 us;
// persistent + register-staged 108 us; XCD-aware 106.5; LDS-direct 104.7; loads interleaved with the MFMA groups 95.5
// (the superseded kernels and the work-queue variant are recorded in profiles/, not kept here).
// (TM = 64 rows per item, K step KT = 32, TrmmItem and TRMM_MAX_ITEMS: sched_host.h)

// ------------------------------------------------------------------------------------------
// LDS-direct variant of the persistent kernel: the k-tiles are streamed from L2 into LDS by
// global_load_lds_dwordx4 (each wave-load lands as one contiguous 1 KiB chunk, lane l -> bytes 16 l .. 16 l + 15),
// so there is no register staging and no ds_write on the waves' instruction streams.  The LDS tiles are
// unpadded, k-major ([k][64] for W, [k][128] for K_*^T); bank conflicts of the fragment reads are avoided by
// storing the odd k-rows with their 16-double blocks swapped (position = index ^ 16) -- the swizzle is applied
// on the GLOBAL side (which pair a lane fetches), the LDS side of a DMA load is always contiguous.  Two LDS
// buffers as distinct arrays (so that hipcc's waitcnt insertion can tell the buffer being filled from the
// one being read); three buffers: the loads of k-tile s+2 are issued at the start of k-tile s and the barrier
// that ends k-tile s waits (s_waitcnt vmcnt(6), written by hand) only for the loads of k-tile s+1.
typedef const __attribute__((address_space(1))) void *gas_ptr;
typedef __attribute__((address_space(3))) void *las_ptr;

// the six loads of k-tile s+2 go out one by one between the MFMA groups of k-tile s
__global__ __launch_bounds__(512, 2) void trmm_vsq_dma_kernel(
    const double *__restrict__ Wt, const double *__restrict__ KS, double *__restrict__ out,
    const TrmmItem *__restrict__ sched, const int *__restrict__ sched_cnt, int max_items,
    int64_t Npad, int64_t Bcap, int k, int nrb,
    // compacted columns (internal.h: LiveCols): sched / sched_cnt hold a schedule for every live block count 0 .. live_max,
    // one after the other, and the launch takes the one of ceil(*live / 64); null: the one schedule there is
    const int *__restrict__ live, int live_max
#ifdef GPEMU_TRMM_STAMPS        // diagnostic build (tools/trmm_balance.py): per-worker time stamps of a launch
    , unsigned long long *__restrict__ stamps
#endif
    ) {
  constexpr int BUFD = KT * TM + KT * TILE;            // one k-tile: [W tile | K_*^T tile], 48 KiB
  __shared__ __attribute__((aligned(16))) double L0[BUFD];
  __shared__ __attribute__((aligned(16))) double L1[BUFD];
  __shared__ __attribute__((aligned(16))) double L2[BUFD];
  __shared__ double red[2][TILE];
  __shared__ TrmmItem s_items[TRMM_MAX_ITEMS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int lr = lane & 15, lk = lane >> 4;

#ifdef GPEMU_TRMM_STAMPS
  if (stamps && tid == 0) stamps[blockIdx.x * 16] = __builtin_amdgcn_s_memrealtime();
#endif
  if (live) {
    int c = (*live + 63) >> 6;
    c = c < 0 ? 0 : (c > live_max ? live_max : c);
    sched += (int64_t)c * gridDim.x * max_items;
    sched_cnt += (int64_t)c * gridDim.x;
  }
  const int nitems = sched_cnt[blockIdx.x];
  if (tid < nitems) s_items[tid] = sched[(int64_t)blockIdx.x * max_items + tid];
  __syncthreads();
  if (nitems == 0) return;
  const TrmmItem *my = s_items;

  // per-lane source offsets (doubles) of the wave's six 1 KiB chunks of a k-tile
  int offA[2], offB[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int kk = 2 * (wave * 2 + j) + (lane >> 5);          // chunk = two k-rows of the W tile
    offA[j] = kk * (int)Npad + ((2 * (lane & 31)) ^ ((kk & 1) << 4));
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kk = wave * 4 + r;                              // chunk = one k-row of the K_*^T tile
    offB[r] = kk * (int)Bcap + ((2 * lane) ^ ((kk & 1) << 4));
  }
  const int64_t astep = (int64_t)KT * Npad, bstep = (int64_t)KT * Bcap;

  // ---- load cursor (one k-tile ahead of the compute cursor) ----
  int l_item = 0, l_t = 0, l_nt = 1;
  const double *l_pa = Wt, *l_pb = KS;
  auto l_open = [&]() {
    const TrmmItem it = my[l_item];
    const int64_t i0 = (int64_t)it.rb * TM;
    l_nt = (int)((i0 + TM + KT - 1) / KT);
    l_pa = Wt + (int64_t)it.p * Npad * Npad + i0;
    l_pb = KS + (int64_t)it.p * Npad * Bcap + (it.col0 & ~(TILE - 1));
    l_t = 0;
  };
  // Issued as inline assembly: with the builtin, hipcc's waitcnt insertion treats every later LDS read as a
  // possible reader of the in-flight destination and drains vmcnt to 0, which defeats the two-tile lookahead;
  // the waits for these loads are the hand-written s_waitcnt vmcnt(6) of tile_barrier().
  auto dma1 = [&](const double *src, double *dst_wave_uniform) {
    const unsigned lds_off = (unsigned)(uintptr_t)((las_ptr)dst_wave_uniform);
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off"
                 :
                 : "s"(lds_off), "v"(src)
                 : "memory");
  };
  // one of the wave's six loads of a k-tile (part compile-time after unrolling); the cursor moves on after the last
  auto dma_part = [&](double *dA, int part) {
    double *dB = dA + KT * TM;
    if (part < 2) dma1(l_pa + offA[part], dA + (wave * 2 + part) * 128);
    else dma1(l_pb + offB[part - 2], dB + (wave * 4 + part - 2) * 128);
    if (part == 5 && l_item < nitems) {
      if (++l_t == l_nt) {
        if (++l_item < nitems) l_open();   // else: stay on the last k-tile (harmless re-read)
      } else {
        l_pa += astep;
        l_pb += bstep;
      }
    }
  };
  auto dma = [&](double *dA) {
#pragma unroll
    for (int part = 0; part < 6; ++part) dma_part(dA, part);
  };

  // vmcnt(6) lgkmcnt(0): everything but this wave's six newest loads has landed, every LDS read has returned
  auto tile_barrier = [&]() {
    __builtin_amdgcn_s_waitcnt(0x0076);
    __builtin_amdgcn_s_barrier();
  };
  l_open();
  dma(L0);
  dma(L1);
  tile_barrier();
#ifdef GPEMU_TRMM_STAMPS
  if (stamps && tid == 0) stamps[blockIdx.x * 16 + 1] = __builtin_amdgcn_s_memrealtime();
#endif

  d4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};

  int c_item = 0, c_t = 0;
  TrmmItem cur = my[0];
  int c_nt = (int)(((int64_t)cur.rb * TM + TM + KT - 1) / KT);
  const int sw = (lk & 1) << 4;                                 // this lane's k-rows are odd <=> lk odd
  const int ia0 = lk * TM + ((wm * 32 + lr) ^ sw), ia1 = lk * TM + ((wm * 32 + 16 + lr) ^ sw);

  auto step = [&](const double *cA, double *nA) -> bool {
    const double *cB = cA + KT * TM;
    if (cur.half) {
      const int ib = lk * TILE + (((cur.col0 & 64) + wn * 16 + lr) ^ sw);
      double a[2][2], b[2];
      a[0][0] = cA[ia0];
      a[0][1] = cA[ia1];
      b[0] = cB[ib];
#pragma unroll
      for (int ks = 0; ks < KT / 4; ++ks) {
        const int cu = ks & 1, nx = cu ^ 1;
        if (ks + 1 < KT / 4) {
          a[nx][0] = cA[(ks + 1) * 4 * TM + ia0];
          a[nx][1] = cA[(ks + 1) * 4 * TM + ia1];
          b[nx] = cB[(ks + 1) * 4 * TILE + ib];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
          acc[mi][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cu][mi], b[cu], acc[mi][0], 0, 0, 0);
        if (ks < 6) dma_part(nA, ks);   // k-tile +2 -> the buffer k-tile -1 was read from
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      const int ib0 = lk * TILE + ((wn * 32 + lr) ^ sw), ib1 = lk * TILE + ((wn * 32 + 16 + lr) ^ sw);
      double a[2][2], b[2][2];
      a[0][0] = cA[ia0];
      a[0][1] = cA[ia1];
      b[0][0] = cB[ib0];
      b[0][1] = cB[ib1];
#pragma unroll
      for (int ks = 0; ks < KT / 4; ++ks) {
        const int cu = ks & 1, nx = cu ^ 1;
        if (ks + 1 < KT / 4) {
          a[nx][0] = cA[(ks + 1) * 4 * TM + ia0];
          a[nx][1] = cA[(ks + 1) * 4 * TM + ia1];
          b[nx][0] = cB[(ks + 1) * 4 * TILE + ib0];
          b[nx][1] = cB[(ks + 1) * 4 * TILE + ib1];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cu][mi], b[cu][ni], acc[mi][ni], 0, 0, 0);
        if (ks < 6) dma_part(nA, ks);   // k-tile +2 -> the buffer k-tile -1 was read from
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    tile_barrier();
    if (++c_t == c_nt) {
      const int ncols = cur.half ? 64 : TILE;
      const int wcol = cur.half ? wn * 16 : wn * 32;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        if (ni == 0 || !cur.half) {
          double sq = 0.0;
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) sq = fma(acc[mi][ni][r], acc[mi][ni][r], sq);
          sq += __shfl_xor(sq, 16);
          sq += __shfl_xor(sq, 32);
          if (lk == 0) red[wm][wcol + ni * 16 + lr] = sq;
        }
      }
      __syncthreads();
      if (tid < ncols)
        out[(((int64_t)cur.col0 + tid) * k + cur.p) * nrb + cur.rb] = red[0][tid] + red[1][tid];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};
#ifdef GPEMU_TRMM_STAMPS
      if (stamps && tid == 0 && c_item < 13) stamps[blockIdx.x * 16 + 2 + c_item] = __builtin_amdgcn_s_memrealtime();
#endif
      if (++c_item == nitems) return true;
      cur = my[c_item];
      c_nt = (int)(((int64_t)cur.rb * TM + TM + KT - 1) / KT);
      c_t = 0;
    }
    return false;
  };
  for (;;) {
    if (step(L0, L2)) break;
    if (step(L1, L0)) break;
    if (step(L2, L1)) break;
  }
}

// host side: the schedule and table builders are in sched_host.h (checked on the CPU by tests/native/sched_host_check.cpp);
// here they are given the model's shape, and their output is cached and uploaded
static_assert(SCHED_TILE == TILE && SCHED_KSTAR_ROWS == KSTAR_ROWS_BIG, "sched_host.h restates internal.h's tile sizes");
static SchedShape sched_shape(const gpemu_model *m) { return SchedShape{(int)m->k, (int)m->vsq_nrb, m->Npad, m->num_cu}; }
static void build_trmm_schedule(gpemu_model *m, int ncb, std::vector<TrmmItem> &flat, std::vector<int> &cnt,
                                int &max_items, int &nworkers, bool (*keep)(int p, int rb) = nullptr, int split_all = 0) {
  build_trmm_schedule(sched_shape(m), ncb, flat, cnt, max_items, nworkers, keep, split_all);
}

// The compacted half-step's tables (sched_host.h: build_live_tables) for batches of ncb 128-column blocks.  Built once per
// (model, shape, form) by the first launch that needs it, like the whole batch's schedule.
static int live_deal(gpemu_model *m, int ncb, int form, hipStream_t st, const gpemu_model::LiveDeal **out) {
  const int cap = m->num_cu;
  for (const auto &e : m->live_cache)
    if (e.ncb == ncb && e.cap == cap && e.form == form) { *out = &e; return GPEMU_OK; }
  LiveTables t;
  const int rc = build_live_tables(sched_shape(m), ncb, form, t);
  if (rc == LIVE_TABLES_NO_MAP) {
    set_error("compacted half-step: %d PCs x %d row chunks x %d column blocks do not fit the cross-kernel's map", (int)m->k,
              (int)(m->Npad / KSTAR_ROWS_BIG), 2 * ncb);
    return GPEMU_ERR_UNSUPPORTED;
  }
  if (rc == LIVE_TABLES_TOO_MANY_ITEMS) {
    set_error("triangular GEMM schedule needs %d items per worker (limit %d): batch too large for one launch", t.full_max_items,
              TRMM_MAX_ITEMS);
    return GPEMU_ERR_UNSUPPORTED;
  }
  const std::vector<TrmmItem> &items = t.items;
  const std::vector<int> &cnt = t.cnt, &kmap = t.kmap;
  const int stride = t.stride, workers = t.workers, nwg = t.nwg;
  DevScope sc(st);   // owns the new entry until it is complete
  TrmmItem *ditems = nullptr;
  int *dcnt = nullptr, *dkmap = nullptr;
  GP_TRY(sc.alloc(&ditems, (int64_t)items.size()));
  GP_TRY(sc.alloc(&dcnt, (int64_t)cnt.size()));
  GP_TRY(sc.alloc(&dkmap, (int64_t)kmap.size()));
  GP_HIP(hipMemcpy(ditems, items.data(), sizeof(TrmmItem) * items.size(), hipMemcpyHostToDevice));
  GP_HIP(hipMemcpy(dcnt, cnt.data(), sizeof(int) * cnt.size(), hipMemcpyHostToDevice));
  GP_HIP(hipMemcpy(dkmap, kmap.data(), sizeof(int) * kmap.size(), hipMemcpyHostToDevice));
  m->live_cache.push_back({ncb, cap, form, sc.release(ditems), sc.release(dcnt), sc.release(dkmap), stride, workers, nwg});
  *out = &m->live_cache.back();
  return GPEMU_OK;
}

int prepare_live_cols(gpemu_model *m, int64_t B, int form, hipStream_t st) {
  const gpemu_model::LiveDeal *deal = nullptr;
  return live_deal(m, (int)(round_up(B, TILE) / TILE), form, st, &deal);
}

static int launch_trmm_vsq_one(gpemu_model *m, int64_t B, hipStream_t st, bool piece, const LiveCols *lv = nullptr);

int launch_trmm_vsq(gpemu_model *m, int64_t B, hipStream_t st, const LiveCols *lv) {
  Workspace &w = m->ws;
  const int64_t per = trmm_piece_cols(m, B);
  if (lv && (per < round_up(B, TILE) || (m->variant_B > 0 ? m->variant_B : B) <= 128)) {
    set_error("compacted columns: the triangular GEMM takes them as one large-batch launch");   // (the sampler's eligibility test)
    return GPEMU_ERR_STATE;
  }
  if (per < round_up(B, TILE)) {     // one launch per piece; the column partials of a piece land where a single launch would put them
    path_count(GPEMU_PATH_TRMM_DMA_PIECES);
    double *const KS0 = w.KS, *const V0 = w.vsq_part;
    int rc = GPEMU_OK;
    for (int64_t c0 = 0; c0 < B && rc == GPEMU_OK; c0 += per) {
      w.KS = KS0 + c0;
      w.vsq_part = V0 + c0 * m->k * m->vsq_nrb;
      rc = launch_trmm_vsq_one(m, std::min(per, B - c0), st, true);
    }
    w.KS = KS0;
    w.vsq_part = V0;
    return rc;
  }
  return launch_trmm_vsq_one(m, B, st, false, lv);
}

// one launch of the triangular GEMM for B columns (a whole batch, or one piece of it)
static int launch_trmm_vsq_one(gpemu_model *m, int64_t B, hipStream_t st, bool piece, const LiveCols *lv) {
  Workspace &w = m->ws;
  constexpr int64_t smallb_max = 128;
  const int64_t Bv = m->variant_B > 0 ? m->variant_B : B;   // a chain stacked with others is evaluated as it would be alone
  if (Bv <= smallb_max) {  // small batch: persistent 32 x 32 items, operands straight into registers
    const int rc = launch_trmm_vsq_small(m, B, st);
    if (rc != GPEMU_ERR_UNSUPPORTED) return rc;
    if (m->variant_B > 0) {
      set_error("stacked chains: the small-batch triangular GEMM cannot take %lld columns", (long long)B);
      return rc;
    }
    // a shape with more items per worker than the small-batch kernel holds: the large-batch kernel with every item halved
    path_count(GPEMU_PATH_TRMM_SMALL_FALLBACK);
  }
  w.cur_nrb = (int)m->vsq_nrb;
  const int nrb = (int)m->vsq_nrb;
  const int ncb = (int)(round_up(B, TILE) / TILE);  // only the column tiles that hold real queries
  const int cap = m->num_cu;
  if (m->sched_ncb != ncb || m->sched_cap != cap) {
    const gpemu_model::SchedEntry *hit = nullptr;
    for (const auto &e : m->sched_cache)
      if (e.ncb == ncb && e.cap == cap) hit = &e;
    if (!hit) {
      std::vector<TrmmItem> flat;
      std::vector<int> cnt;
      int max_items = 0, nworkers = 0;
      build_trmm_schedule(m, ncb, flat, cnt, max_items, nworkers);
      if (max_items > TRMM_MAX_ITEMS) {
        set_error("triangular GEMM schedule needs %d items per worker (limit %d): batch too large for one launch",
                  max_items, TRMM_MAX_ITEMS);
        return GPEMU_ERR_UNSUPPORTED;
      }
      // schedules are kept (a few KB each): launches in flight keep reading the one they were given
      DevScope sc(st);   // owns the new entry until it is complete
      TrmmItem *ditems = nullptr;
      int *dcnt = nullptr;
      GP_TRY(sc.alloc(&ditems, (int64_t)flat.size()));
      GP_TRY(sc.alloc(&dcnt, (int64_t)cnt.size()));
      GP_HIP(hipMemcpy(ditems, flat.data(), sizeof(TrmmItem) * flat.size(), hipMemcpyHostToDevice));
      GP_HIP(hipMemcpy(dcnt, cnt.data(), sizeof(int) * cnt.size(), hipMemcpyHostToDevice));
      m->sched_cache.push_back({ncb, cap, sc.release(ditems), sc.release(dcnt), max_items, nworkers});
      hit = &m->sched_cache.back();
    }
    m->sched_items = hit->items; m->sched_cnt = hit->cnt;
    m->sched_ncb = ncb; m->sched_cap = cap; m->sched_max_items = hit->max_items; m->sched_workers = hit->workers;
  }
  if (!piece) path_count(GPEMU_PATH_TRMM_DMA_WHOLE);
  // build_trmm_schedule's XCD-aware placement: every CU a worker, whole groups per XCD
  const bool xcd = m->sched_workers == cap && cap % 8 == 0 && ((int)m->k * ncb) % 8 == 0;
  path_count(xcd ? GPEMU_PATH_TRMM_DMA_XCD : GPEMU_PATH_TRMM_DMA_LPT);
  // compacted columns: the schedules of every live block count, the launch's own picked on the device; the grid, the
  // path counters and the event pair are the whole batch's
  const TrmmItem *items = (const TrmmItem *)m->sched_items;
  const int *cnts = m->sched_cnt, *live = nullptr;
  int max_items = m->sched_max_items, workers = m->sched_workers;
  if (lv) {
    const gpemu_model::LiveDeal *deal = nullptr;
    GP_TRY(live_deal(m, ncb, lv->form, st, &deal));
    items = (const TrmmItem *)deal->items; cnts = deal->cnt; max_items = deal->max_items; workers = deal->workers;
    live = lv->n_live;
  }
  const int pe0 = prof_mark(m, st);
#ifdef GPEMU_TRMM_STAMPS
  // diagnostic build only (make STAMPS=1; tools/trmm_balance.py): per-worker time stamps of launch 600, dumped to the
  // file GPEMU_TRMM_STAMP_FILE names.  The product build has neither the state nor the getenv in its launch path.
  static const char *stamp_path = getenv("GPEMU_TRMM_STAMP_FILE");
  static unsigned long long *dstamps = nullptr;
  static int stamp_calls = 0;
  if (stamp_path && !dstamps) {
    GP_TRY(dev_alloc(&dstamps, 16 * 1024));
    GP_HIP(hipMemset(dstamps, 0, sizeof(unsigned long long) * 16 * 1024));
  }
  hipLaunchKernelGGL(trmm_vsq_dma_kernel, dim3((unsigned)workers), dim3(512), 0, st, m->Wt,
                     w.KS, w.vsq_part, items, cnts, max_items,
                     m->Npad, w.Bcap, (int)m->k, nrb, live, 2 * ncb, dstamps);
  GP_HIP(hipGetLastError());
  prof_pair(m, 0, pe0, prof_mark(m, st));
  if (stamp_path && ++stamp_calls == 600) {
    GP_HIP(hipStreamSynchronize(st));
    std::vector<unsigned long long> h(16 * 1024);
    GP_HIP(hipMemcpy(h.data(), dstamps, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    std::vector<int> cnt(m->sched_workers);
    GP_HIP(hipMemcpy(cnt.data(), m->sched_cnt, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
    if (FILE *f = fopen(stamp_path, "w")) {
      unsigned long long t0 = ~0ull;
      for (int wk = 0; wk < m->sched_workers; ++wk) t0 = std::min(t0, h[wk * 16]);
      for (int wk = 0; wk < m->sched_workers; ++wk) {
        fprintf(f, "%d %d", wk, cnt[wk]);
        for (int i = 0; i < 2 + std::min(cnt[wk], 12); ++i) fprintf(f, " %.2f", (double)(h[wk * 16 + i] - t0) / 100.0);
        fprintf(f, "\n");
      }
      fclose(f);
    }
  }
#else
  hipLaunchKernelGGL(trmm_vsq_dma_kernel, dim3((unsigned)workers), dim3(512), 0, st, m->Wt,
                     w.KS, w.vsq_part, items, cnts, max_items,
                     m->Npad, w.Bcap, (int)m->k, nrb, live, 2 * ncb);
  GP_HIP(hipGetLastError());
  prof_pair(m, 0, pe0, prof_mark(m, st));
#endif
  return GPEMU_OK;
}

// ------------------------------------------------------------------------------------------
__global__ void reduce_mean_var_kernel(const double *__restrict__ mean_part,
                                       const double *__restrict__ vsq_part,
                                       const double *__restrict__ kdiag, double *__restrict__ mean,
                                       double *__restrict__ var, int64_t B, int64_t Bcap, int k,
                                       int nchunk, int nrb) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * k) return;
  int p = (int)(idx / B);
  int64_t b = idx - (int64_t)p * B;
  double mu = 0.0, vs = 0.0;
  for (int c = 0; c < nchunk; ++c) mu += mean_part[(b * k + p) * nchunk + c];
  for (int r = 0; r < nrb; ++r) vs += vsq_part[(b * k + p) * nrb + r];
  double v = kdiag[p] - vs;
  if (v < 0.0) v = 0.0;     // skl _gpr.py:479-485
  double sd = sqrt(v);      // predict returns std (skl _gpr.py:494) ...
  mean[b * k + p] = mu;
  var[b * k + p] = sd * sd; // ... and the reference squares it again (ref: emulation.py:499)
}

int launch_reduce_mean_var(gpemu_model *m, int64_t B, double *dmean, double *dvar, hipStream_t st) {
  const Workspace &w = m->ws;
  int64_t n = B * m->k;
  hipLaunchKernelGGL(reduce_mean_var_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     w.mean_part, w.vsq_part, m->kdiag, dmean, dvar, B, w.Bcap, (int)m->k,
                     w.cur_nchunk, w.cur_nrb);
  GP_HIP(hipGetLastError());
  return GPEMU_OK;
}

}  // namespace gpemu
