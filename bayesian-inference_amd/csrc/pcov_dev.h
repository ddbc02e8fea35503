// What the joint predictive covariance (k_pcov.hip) shares with the sequential design (k_design.hip;
// DESIGN 4.32): the kernel value of a pair of raw rows, the launch of a block of kernel values per PC, and V = W K^T.
#pragma once
#include "internal.h"
#include "matern_dev.h"

namespace gpemu {

constexpr int PC_NB = 64;   // padding unit of every operand (launch_gemm, the blocked Cholesky)

// one block of kernel values per PC: out[z][r][c] = k(A[a0 + r], B[b0 + c]) + const for a0 + r < na, b0 + c < nb;
// zero in the padding.  sym: element (i, i) is kernel_.diag exactly (r = 0: 1 + const + noise).
struct KmatArgs {
  const double *A = nullptr;   // rows [na][sa] (raw coordinates, first d columns read)
  const double *B = nullptr;   // rows [nb][sb]
  int64_t sa = 0, sb = 0, na = 0, nb = 0, a0 = 0, b0 = 0;
  double *out = nullptr;
  int64_t ldo = 0, strideo = 0, rows = 0, cols = 0;   // rows, cols: multiples of 16 and 64
  const double *ls = nullptr;      // [k][dp]
  const double *constv = nullptr;  // [k]
  const double *kdiag = nullptr;   // [k]
  int dp = DPAD, d = 1, p0 = 0, sym = 0;
  MaternNu mn;
};

#if defined(__HIPCC__)
// k(a, b) + const of one pair of raw rows: the direct distance r^2 = sum_i ((a_i - b_i) (1 / ls_i))^2, the library exp
// of the closed forms or the out-of-line general-nu call.  The one copy of these numerics: cov_ref's bound is for them.
template <int KIND, int DP>
__device__ __forceinline__ double kmat_value(const double *a, const double *xb, const double *inv, int d,
                                             const MaternNu &mn, double cst) {
  double r2 = 0.0;
#pragma unroll
  for (int dd = 0; dd < DP; ++dd) {
    if (dd < d) {
      const double df = (a[dd] - xb[dd]) * inv[dd];
      r2 = fma(df, df, r2);
    }
  }
  const double r = sqrt(r2);   // before the call copies mn (the other order changes the instruction schedule)
  return (KIND == 4 ? matern_nu_value_call(mn, r) : base_from_r2(KIND, r2)) + cst;
}
#endif

// the block of g for the PCs [g.p0, g.p0 + npc) of m (k_pcov.hip); asynchronous on st
int launch_kmat(const gpemu_model *m, KmatArgs g, int npc, hipStream_t st);
// V[z] = W_p KT[z]  (W = Wt^T lower triangular: k_to_m skips the tiles above the diagonal), rows [0, N64) of each PC's
// block of V, which starts strideV elements after the one before (0: N64 * ncols, the blocks back to back)
int launch_v(const gpemu_model *m, int p0, int npc, const double *KT, double *V, int64_t N64, int64_t ncols,
             hipStream_t st, int64_t strideV = 0);

}  // namespace gpemu
