// Row-wise log-sum-exp of pairwise Gaussian log-weights (gpemu_pair_lse*): the inner sum of the nested
// Monte Carlo estimator of the expected information gain of a candidate measurement.
//
// For rows Y [n][F] and Z [S][F], a_ij = -|y_i - z_j|^2 / 2, and per row i: m_i = max_j a_ij, s1_i = sum_j exp(a_ij - m_i),
// s2_i = sum_j exp(2 (a_ij - m_i)); lse_i = m_i + log s1_i, ess_i = s1_i^2 / s2_i.  The n x S matrix never exists.
//
// pairlse_centre_kernel: the pre-pass.  One thread per row subtracts the centre (one rounded operation per element),
// writes the row FEATURE-MAJOR ([feature][row], rows padded to the tile, features padded with zeros to a whole k-tile)
// and its half squared norm h = |x - c|^2 / 2 as one fma chain over the features in increasing order.  A padding row
// gets zeros and h = +inf: its every a is -inf, its weight exactly 0 -- the partial kernel needs no bounds test.
//
// pairlse_partial_kernel: workgroup (chunk of PL_CHUNK columns of Z, block of PL_ROWS = 64 rows of Y), 256 threads =
// 2 x 2 waves, each a 32 x 64 quarter of a 64 x PL_T tile of the y.z products.  Both operands go through LDS in
// k-tiles of PL_GK features ([k][cols + 16] doubles: the k-rows lie 16 mod 32 doubles apart, as in k_kde2d.hip), the
// next k-tile is fetched into registers while v_mfma_f64_16x16x4_f64 runs on the current one.  Only ceil(F / 4) k-steps
// are issued: the MFMA chain has length 4 ceil(F / 4), and the padding zeros add exactly.  Epilogue of a tile:
// a = (y.z - h_i) - h_j, the excluded pair (i, self[i]) set to -inf; every lane keeps an online (m, s1, s2) for each of
// its 8 rows and rescales at most once per tile: one exp per pair plus one per row and tile.  At the end of the chunk
// the 16 lanes that share a row are merged by the xor butterfly 1, 2, 4, 8, then the two waves that share it (columns
// 0 .. 63 of every tile first), and the chunk's (m, s1, s2) is stored.
//
// pairlse_merge_kernel: one thread per row merges its chunks' triples in chunk order and writes lse and ess.
//
// No floating-point atomics.  A chunk is PL_CHUNK columns whatever n, the grid or the workspace: every output has the
// same bits for every batching of the row blocks and every run.
#include <algorithm>
#include <cmath>
#include <vector>

#include "internal.h"
#include "rows_dev.h"
#include "wave_dev.h"

namespace gpemu {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int PL_ROWS = GPEMU_PAIRLSE_TILE_ROWS;   // rows of Y per workgroup
constexpr int PL_T = 128;                          // columns of Z per tile
constexpr int PL_GK = 16;                          // features per k-tile
constexpr int PL_SKY = PL_ROWS + 16;               // an operand k-row in LDS: 16 mod 32 doubles apart
constexpr int PL_SKZ = PL_T + 16;
constexpr int PL_CHUNK = GPEMU_PAIRLSE_CHUNK;      // columns per partial triple
constexpr int PL_MAX_F = 65536;
static_assert(PL_ROWS == 64 && PL_CHUNK % PL_T == 0 && PL_SKY % 32 == 16 && PL_SKZ % 32 == 16, "the tile's shape");

static inline void pairlse_path_count(int path) { count_path(PATHS_PAIRLSE, path); }   // enum gpemu_pairlse_path

// (m, s1, s2) of a set of log-weights: s1 = sum exp(a - m), s2 = sum exp(2 (a - m)); the empty set is (-inf, 0, 0)
struct Lse3 { double m, s1, s2; };

// the union of two sets, a first.  One of the two factors is exp(0) = 1 exactly; an empty side adds exactly 0 and two
// empty sides stay empty: -inf - (-inf) is never formed
static __device__ __forceinline__ Lse3 lse3_merge(const Lse3 &a, const Lse3 &b) {
#pragma clang fp contract(off)   // a sum of two rounded products: the same bits whichever side is `a`
  const double M = fmax(a.m, b.m);
  if (!(M > -INFINITY)) return Lse3{-INFINITY, 0.0, 0.0};
  const double ea = exp(a.m - M), eb = exp(b.m - M);
  const double pa1 = a.s1 * ea, pb1 = b.s1 * eb, pa2 = (a.s2 * ea) * ea, pb2 = (b.s2 * eb) * eb;
  return Lse3{M, pa1 + pb1, pa2 + pb2};
}

// ---- pre-pass -------------------------------------------------------------------------------------------------------
// rows [r0, r0 + npad) of X [n][ld] (F columns) minus centre, feature-major into Xt [Fp][npad], h [npad]; thread per row
__global__ __launch_bounds__(256) void pairlse_centre_kernel(const double *__restrict__ X, int64_t ld, int64_t n, int64_t r0,
                                                             int64_t npad, int F, int Fp, const double *__restrict__ centre,
                                                             double *__restrict__ Xt, double *__restrict__ h) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  const int64_t r = r0 + i;
  const bool live = r < n;
  const double *row = X + (live ? r : 0) * ld;
  double acc = 0.0;
  for (int f = 0; f < F; ++f) {
    const double c = live ? row[f] - centre[f] : 0.0;
    Xt[(int64_t)f * npad + i] = c;
    acc = fma(c, c, acc);
  }
  for (int f = F; f < Fp; ++f) Xt[(int64_t)f * npad + i] = 0.0;
  h[i] = live ? 0.5 * acc : INFINITY;
}

// ---- the partial kernel ---------------------------------------------------------------------------------------------
struct PairLseArgs {
  const double *Yt, *hy;     // [Fp][ldy] centred rows of the batch, feature-major; [ldy]; ldy = 64 (row blocks of the batch)
  const double *Zt, *hz;     // [Fp][ldz]; [ldz]; ldz = S rounded up to PL_T
  const int64_t *self;       // [n] (all rows), or null
  int64_t ldy, ldz, n, row0; // row0: the first row of the batch
  int64_t S, nchunk;
  int nkt, F4;               // k-tiles (Fp / PL_GK); F rounded up to 4
  double *part;              // [row blocks of the batch][nchunk][3][64]
};

__global__ __launch_bounds__(256, 2) void pairlse_partial_kernel(PairLseArgs g) {
  __shared__ __attribute__((aligned(16))) double pl_lds[2 * PL_GK * (PL_SKY + PL_SKZ)];
  double *sY = pl_lds, *sZ = pl_lds + 2 * PL_GK * PL_SKY;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lk = lane >> 4;
  const int64_t c = blockIdx.x, rb = blockIdx.y;
  const int64_t j0 = c * PL_CHUNK, j1 = (j0 + PL_CHUNK < g.S) ? j0 + PL_CHUNK : g.S;
  const int ntile = (int)((j1 - j0 + PL_T - 1) / PL_T), nkt = g.nkt, nstep = ntile * nkt;

  // the loads of a k-tile: thread (column yc, k-rows ykq + 4 j) of Y's 64 x 16, (column zc, k-rows zkq + 2 j) of Z's
  // 128 x 16; consecutive lanes read consecutive doubles.  Every address is inside the padded buffers: rb 64 + yc < ldy,
  // and a tile starts below S at a multiple of PL_T, so its 128 columns end within ldz
  const int yc = tid & 63, ykq = tid >> 6, zc = tid & 127, zkq = tid >> 7;
  const double *gy = g.Yt + rb * PL_ROWS + yc, *gz = g.Zt + j0 + zc;
  double ry[4], rz[8];
  auto gload = [&](int step) {
    const int jt = step / nkt, kt = step - jt * nkt;
#pragma unroll
    for (int j = 0; j < 4; ++j) ry[j] = gy[(int64_t)(kt * PL_GK + ykq + 4 * j) * g.ldy];
#pragma unroll
    for (int j = 0; j < 8; ++j) rz[j] = gz[(int64_t)(kt * PL_GK + zkq + 2 * j) * g.ldz + (int64_t)jt * PL_T];
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) sY[buf * PL_GK * PL_SKY + (ykq + 4 * j) * PL_SKY + yc] = ry[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) sZ[buf * PL_GK * PL_SKZ + (zkq + 2 * j) * PL_SKZ + zc] = rz[j];
  };

  // this lane's rows: wm 32 + mi 16 + lk + 4 r of the block (the accumulator layout of the 16 x 16 tiles)
  double hy[2][4];
  int sj[2][4];
  Lse3 st[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t lrow = rb * PL_ROWS + wm * 32 + mi * 16 + lk + 4 * r, row = g.row0 + lrow;
      hy[mi][r] = g.hy[lrow];
      sj[mi][r] = (g.self && row < g.n) ? (int)g.self[row] : -1;
      st[mi][r] = Lse3{-INFINITY, 0.0, 0.0};
    }

  d4 acc[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};

  gload(0);
  sstore(0);
  __syncthreads();
  for (int step = 0; step < nstep; ++step) {
    const int buf = step & 1, jt = step / nkt, kt = step - jt * nkt;
    const double *bY = sY + buf * PL_GK * PL_SKY, *bZ = sZ + buf * PL_GK * PL_SKZ;
    if (step + 1 < nstep) gload(step + 1);
    const int nks = (g.F4 - kt * PL_GK >= PL_GK) ? PL_GK / 4 : (g.F4 - kt * PL_GK) / 4;
#pragma unroll
    for (int ks = 0; ks < PL_GK / 4; ++ks) {
      if (ks < nks) {
        double a[2], b[4];
        const int kk = ks * 4 + lk;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) a[mi] = bY[kk * PL_SKY + wm * 32 + mi * 16 + lr];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) b[ni] = bZ[kk * PL_SKZ + wn * 64 + ni * 16 + lr];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
      }
    }
    if (kt + 1 == nkt) {
      // the tile is complete: D[reg] is row (lane >> 4) + 4 reg, column lane & 15 of each 16 x 16 tile
      const int64_t cb = j0 + (int64_t)jt * PL_T + wn * 64 + lr;
      double hz[4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) hz[ni] = g.hz[cb + 16 * ni];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double a[4], tm = -INFINITY;
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            double v = (acc[mi][ni][r] - hy[mi][r]) - hz[ni];
            if ((int)(cb + 16 * ni) == sj[mi][r]) v = -INFINITY;
            a[ni] = v;
            tm = fmax(tm, v);
          }
          Lse3 &t = st[mi][r];
          if (tm > t.m) {   // (at most once per tile; from the empty state: exp(-inf) = 0 times 0)
            const double sc = exp(t.m - tm);
            t.s1 *= sc;
            t.s2 *= sc * sc;
            t.m = tm;
          }
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            const double e = (a[ni] > -INFINITY) ? exp(a[ni] - t.m) : 0.0;
            t.s1 += e;
            t.s2 = fma(e, e, t.s2);
          }
        }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};
    }
    if (step + 1 < nstep) sstore(buf ^ 1);
    __syncthreads();
  }

  // the 16 lanes of a row: butterfly over lane & 15 (every lane ends with the same triple); then the two waves of a row
  // block half through LDS (free: the loop ended in a barrier), columns 0 .. 63 of the tiles first
  double *sm = pl_lds;   // [2 (wm)][3][32]
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Lse3 t = st[mi][r];
#pragma unroll
      for (int off = 1; off <= 8; off <<= 1) {
        const Lse3 o{__shfl_xor(t.m, off, 64), __shfl_xor(t.s1, off, 64), __shfl_xor(t.s2, off, 64)};
        t = (lr & off) ? lse3_merge(o, t) : lse3_merge(t, o);
      }
      st[mi][r] = t;
      if (wn == 1 && lr == 0) {
        const int q = mi * 16 + lk + 4 * r;
        sm[(wm * 3 + 0) * 32 + q] = t.m;
        sm[(wm * 3 + 1) * 32 + q] = t.s1;
        sm[(wm * 3 + 2) * 32 + q] = t.s2;
      }
    }
  __syncthreads();
  if (wn == 0 && lr == 0) {
    double *out = g.part + (rb * g.nchunk + c) * (3 * PL_ROWS);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = mi * 16 + lk + 4 * r;
        const Lse3 o{sm[(wm * 3 + 0) * 32 + q], sm[(wm * 3 + 1) * 32 + q], sm[(wm * 3 + 2) * 32 + q]};
        const Lse3 t = lse3_merge(st[mi][r], o);
        out[0 * PL_ROWS + wm * 32 + q] = t.m;
        out[1 * PL_ROWS + wm * 32 + q] = t.s1;
        out[2 * PL_ROWS + wm * 32 + q] = t.s2;
      }
  }
}

// lse[i], ess[i] (or null) of the nb rows of a batch from their chunks' triples, in chunk order; thread per row
__global__ __launch_bounds__(256) void pairlse_merge_kernel(const double *__restrict__ part, int64_t nchunk, int64_t nb,
                                                            double *__restrict__ lse, double *__restrict__ ess) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const double *p = part + (i / PL_ROWS) * nchunk * (3 * PL_ROWS) + (i % PL_ROWS);
  Lse3 t{p[0], p[PL_ROWS], p[2 * PL_ROWS]};
  for (int64_t c = 1; c < nchunk; ++c) {
    const double *q = p + c * (3 * PL_ROWS);
    t = lse3_merge(t, Lse3{q[0], q[PL_ROWS], q[2 * PL_ROWS]});
  }
  lse[i] = t.s1 > 0.0 ? t.m + log(t.s1) : -INFINITY;
  if (ess) ess[i] = t.s1 > 0.0 ? (t.s1 * t.s1) / t.s2 : 0.0;
}

// ---- host -----------------------------------------------------------------------------------------------------------
static int pairlse_check(int64_t n, int64_t S, int64_t F, const void *Y, const void *Z, int64_t ldy, int64_t ldz,
                         int64_t workspace_bytes, const void *lse) {
  GP_ARG(n >= 1 && n < (1ll << 31), "n must be in [1, 2^31)");
  GP_ARG(S >= 1 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(F >= 1 && F <= PL_MAX_F, "F must be in [1, 65536]");
  GP_ARG(Y && Z && lse, "null pointer");
  GP_ARG(ldy >= F && ldz >= F, "a leading dimension must be at least F");
  GP_ARG(workspace_bytes >= 0, "workspace_bytes must be >= 0");
  return GPEMU_OK;
}

static int pairlse_self_check(int64_t n, int64_t S, const int64_t *self) {
  if (self)
    for (int64_t i = 0; i < n; ++i) GP_ARG(self[i] >= -1 && self[i] < S, "every self index must be in [-1, S)");
  return GPEMU_OK;
}

// dcentre[F] = the column means of dZ [S][ldz]: the pooled-moments kernel over the rows as a view
static int pairlse_centre(const double *dZ, int64_t ldz, int64_t S, int F, double *dcentre, DevScope &sc, hipStream_t st) {
  double *dpart = nullptr;
  GP_TRY(sc.alloc(&dpart, (S + MOM_ROWS - 1) / MOM_ROWS * F));
  return launch_pooled_mean(RowsView{dZ, S, 1, ldz, F}, dpart, dcentre, st);
}

// everything on the device; waits for st
static int pairlse_rows(int64_t n, int64_t S, int F, const double *dY, int64_t ldy, const double *dZ, int64_t ldz,
                        const int64_t *dself, const double *dcentre, int64_t workspace_bytes, double *dlse, double *dess,
                        hipStream_t st) {
  const int Fp = (int)round_up(F, PL_GK);
  const int64_t Spad = round_up(S, PL_T), nchunk = (S + PL_CHUNK - 1) / PL_CHUNK, nrb = (n + PL_ROWS - 1) / PL_ROWS;
  int64_t budget = 0;
  GP_TRY(workspace_budget(workspace_bytes, &budget));
  const int64_t per_block = GPEMU_PAIRLSE_BLOCK_BYTES(S, F);
  const int64_t cap = std::min<int64_t>(std::min<int64_t>(nrb, budget / per_block), 65535);
  if (cap < 1) {
    set_error("pair_lse: out of memory: one block of 64 rows (S = %lld, F = %d) needs %lld bytes; %lld bytes %s",
              (long long)S, F, (long long)per_block, (long long)budget, workspace_budget_name(workspace_bytes));
    return GPEMU_ERR_HIP;
  }
  DevScope sc(st);
  double *cen = nullptr, *Zt = nullptr, *hz = nullptr, *Yt = nullptr, *hy = nullptr, *part = nullptr;
  if (!dcentre) {
    GP_TRY(sc.alloc(&cen, F));
    GP_TRY(pairlse_centre(dZ, ldz, S, F, cen, sc, st));
    dcentre = cen;
  }
  GP_TRY(sc.alloc(&Zt, (int64_t)Fp * Spad));
  GP_TRY(sc.alloc(&hz, Spad));
  GP_TRY(sc.alloc(&Yt, (int64_t)Fp * PL_ROWS * cap));
  GP_TRY(sc.alloc(&hy, PL_ROWS * cap));
  GP_TRY(sc.alloc(&part, cap * nchunk * 3 * PL_ROWS));
  pairlse_path_count(GPEMU_PAIRLSE_PATH_CENTRE);
  hipLaunchKernelGGL(pairlse_centre_kernel, dim3((unsigned)((Spad + 255) / 256)), dim3(256), 0, st, dZ, ldz, S, (int64_t)0,
                     Spad, F, Fp, dcentre, Zt, hz);
  GP_HIP(hipGetLastError());
  PairLseArgs a;
  a.Yt = Yt; a.hy = hy; a.Zt = Zt; a.hz = hz; a.self = dself; a.ldz = Spad; a.n = n; a.S = S; a.nchunk = nchunk;
  a.nkt = Fp / PL_GK; a.F4 = (int)round_up(F, 4); a.part = part;
  for (int64_t b0 = 0; b0 < nrb; b0 += cap) {
    const int64_t nbk = std::min(cap, nrb - b0), r0 = b0 * PL_ROWS, npad = nbk * PL_ROWS, nb = std::min(npad, n - r0);
    pairlse_path_count(GPEMU_PAIRLSE_PATH_ROW_BATCH);
    pairlse_path_count(GPEMU_PAIRLSE_PATH_CENTRE);
    hipLaunchKernelGGL(pairlse_centre_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, dY, ldy, n, r0, npad,
                       F, Fp, dcentre, Yt, hy);
    GP_HIP(hipGetLastError());
    a.ldy = npad; a.row0 = r0;
    pairlse_path_count(GPEMU_PAIRLSE_PATH_PARTIAL);
    hipLaunchKernelGGL(pairlse_partial_kernel, dim3((unsigned)nchunk, (unsigned)nbk), dim3(256), 0, st, a);
    GP_HIP(hipGetLastError());
    pairlse_path_count(GPEMU_PAIRLSE_PATH_MERGE);
    hipLaunchKernelGGL(pairlse_merge_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, (const double *)part,
                       nchunk, nb, dlse + r0, dess ? dess + r0 : (double *)nullptr);
    GP_HIP(hipGetLastError());
  }
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

}  // namespace gpemu

using namespace gpemu;

extern "C" {

int gpemu_pairlse_path_counts(int64_t *out, int64_t n) { return read_path_counts(PATHS_PAIRLSE, out, n); }

int gpemu_pair_lse_dev(int device, int64_t n, int64_t S, int64_t F, const double *dY, int64_t ldy, const double *dZ,
                       int64_t ldz, const int64_t *dself, const double *dcentre, int64_t workspace_bytes, double *dlse,
                       double *dess, void *stream) {
  GP_TRY(pairlse_check(n, S, F, dY, dZ, ldy, ldz, workspace_bytes, dlse));
  GP_TRY(device_ready(device));
  hipStream_t st = (hipStream_t)stream;
  if (dself) {   // the indices are checked on the host: a copy, no launch
    std::vector<int64_t> hs((size_t)n);
    GP_HIP(hipMemcpyAsync(hs.data(), dself, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    GP_TRY(pairlse_self_check(n, S, hs.data()));
  }
  return pairlse_rows(n, S, (int)F, dY, ldy, dZ, ldz, dself, dcentre, workspace_bytes, dlse, dess, st);
}

int gpemu_pair_lse(int device, int64_t n, int64_t S, int64_t F, const double *Y, const double *Z, const int64_t *self,
                   const double *centre, int64_t workspace_bytes, double *lse, double *ess) {
  GP_TRY(pairlse_check(n, S, F, Y, Z, F, F, workspace_bytes, lse));
  GP_TRY(pairlse_self_check(n, S, self));
  GP_TRY(device_ready(device));
  hipStream_t st = nullptr;
  DevScope sc(st);
  double *dY = nullptr, *dZ = nullptr, *dcen = nullptr, *dlse = nullptr, *dess = nullptr;
  int64_t *dself = nullptr;
  GP_TRY(sc.alloc(&dY, n * F));
  GP_TRY(sc.alloc(&dZ, S * F));
  GP_TRY(sc.alloc(&dlse, n));
  GP_TRY(upload(dY, Y, n * F, st));
  GP_TRY(upload(dZ, Z, S * F, st));
  if (self) {
    GP_TRY(sc.alloc(&dself, n));
    GP_TRY(upload(dself, self, n, st));
  }
  if (centre) {
    GP_TRY(sc.alloc(&dcen, F));
    GP_TRY(upload(dcen, centre, F, st));
  }
  if (ess) GP_TRY(sc.alloc(&dess, n));
  GP_TRY(pairlse_rows(n, S, (int)F, dY, F, dZ, F, dself, dcen, workspace_bytes, dlse, dess, st));
  GP_TRY(sc.download(lse, dlse, n));
  if (ess) GP_TRY(sc.download(ess, dess, n));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

int gpemu_pairlse_centre_dev(int device, int64_t S, int64_t F, const double *dZ, int64_t ldz, double *dcentre, void *stream) {
  GP_ARG(S >= 1 && S < (1ll << 31), "S must be in [1, 2^31)");
  GP_ARG(F >= 1 && F <= PL_MAX_F, "F must be in [1, 65536]");
  GP_ARG(dZ && dcentre, "null pointer");
  GP_ARG(ldz >= F, "a leading dimension must be at least F");
  GP_TRY(device_ready(device));
  hipStream_t st = (hipStream_t)stream;
  DevScope sc(st);
  GP_TRY(pairlse_centre(dZ, ldz, S, (int)F, dcentre, sc, st));
  GP_HIP(hipStreamSynchronize(st));
  return GPEMU_OK;
}

}  // extern "C"
