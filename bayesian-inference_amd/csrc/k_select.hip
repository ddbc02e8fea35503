// Exact selection in many rows at once, by count or by weight (select_rows of rows_dev.h): what
// gpemu_select*, the posterior-predictive bands (k_postpred.hip) and gpemu_weighted_select* (k_reweight.hip) run.
//
// Radix select on the order-preserving 64-bit key of a double (sel_key), most significant byte first, SEL_PASSES = 8
// passes of 8 bits.  A "row" of the state is a (weight row, value row) pair; a target t >= 1 asks for the smallest
// element at which the cumulative weight reaches t.  Without weights every element weighs 1 and there is one weight
// row: target t is the order statistic of rank t - 1.  Per pass
//   sel_hist_kernel   every workgroup adds a fixed slice of one value row into LDS histograms (LDS integer atomics, the
//                     lanes of a wave that agree with its first lane added as one) and adds its non-zero bins to the
//                     pair's global histogram (64-bit integer atomics: no floating-point sum anywhere).  Counted form:
//                     32-bit LDS bins, a ballot and a popcount.  Weighted form: 64-bit LDS bins and a wave sum; a
//                     sample's weight is loaded only when its key matches a live prefix, and a weight of 0 adds nothing;
//   sel_scan_kernel   per pair, every target walks its histogram to the first bin whose cumulative weight reaches it,
//                     extends its prefix by that digit and keeps the target within the bin.
// All targets of a pair share the passes: they are sorted on the host, so targets with one prefix are neighbours and
// share a "slot" (one histogram); an element is counted in the slot whose prefix it matches, if any.  After the last pass
// the prefix IS the key of the wanted element -- an element of the input, not an approximation.  The pass count is fixed:
// a row of equal values, or of values that differ in the last bits only, takes the same eight passes.  The histograms
// hold integers (every sum of a row's weights is below 2^53), so the result does not depend on the grid, on the slices,
// on the batches or on the order in which workgroups arrive.  A row with a NaN returns NaN for every target
// (np.quantile), and so does a target above the row's total weight; -0 and +0 are distinct keys next to each other, so
// either may be returned for a zero.  More than SEL_MAXT targets go in groups of SEL_MAXT, pairs in batches.
#include <algorithm>
#include <numeric>
#include <type_traits>
#include <vector>

#include "internal.h"
#include "rows_dev.h"
#include "sampler_internal.h"
#include "wave_dev.h"

namespace gpemu {

constexpr int SEL_PASSES = 8;        // 8 bits each
constexpr int64_t SEL_SLICE = 4096;  // least elements per workgroup
constexpr int64_t SEL_MAX_WG = 8192; // workgroups per launch, about

struct SelState {
  u64 *prefix = nullptr;    // [rows][SEL_MAXT] key bits found so far, per target
  u64 *trem = nullptr;      // [rows][SEL_MAXT] target within the weight of the elements that match the prefix, >= 1
  u64 *slotpre = nullptr;   // [rows][SEL_MAXT] prefix of each slot
  int *slot = nullptr;      // [rows][SEL_MAXT] slot of each target
  int *over = nullptr;      // [rows][SEL_MAXT] the target is 0 or above the row's total weight
  int *nslot = nullptr;     // [rows]
  int *nan = nullptr;       // [rows] the value row holds a NaN
  u64 *hist = nullptr;      // [rows][SEL_MAXT][SEL_BINS] weight sums, zero between passes
};

// pair c0 + rl = (weight row w, value row v) = ((c0 + rl) / R_v, (c0 + rl) % R_v); targets: [R_w][nt_all] sorted per row
__global__ __launch_bounds__(256) void sel_init_kernel(SelState s, int rows, int nt, const u64 *__restrict__ targets,
                                                       int64_t nt_all, int64_t c0, int64_t R_v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * SEL_MAXT) return;
  const int t = i % SEL_MAXT, rl = i / SEL_MAXT;
  const int64_t w = (c0 + rl) / R_v;
  const u64 tg = t < nt ? targets[w * nt_all + t] : 1;
  s.prefix[i] = 0;
  s.slotpre[i] = 0;
  s.trem[i] = tg;
  s.over[i] = tg == 0;
  s.slot[i] = 0;
  if (t == 0) {
    s.nslot[rl] = 1;
    s.nan[rl] = 0;
  }
}

// workgroup (pair rl, slice c) of the batch: elements [c slice, (c + 1) slice) of the value row.  WEIGHTED: the weights
// are q (else 1, and the pair is the value row c0 + rl)
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void sel_hist_kernel(SelState s, const double *__restrict__ V, int64_t row_stride,
                                                       int64_t elem_stride, int64_t S, const u64 *__restrict__ q,
                                                       int64_t ldq, int64_t c0, int64_t R_v, int nblk, int64_t slice,
                                                       int pass) {
  typedef typename std::conditional<WEIGHTED, u64, unsigned>::type bin_t;
  __shared__ bin_t h[SEL_MAXT * SEL_BINS];
  __shared__ u64 spre[SEL_MAXT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t rl = blockIdx.x / nblk, c = blockIdx.x % nblk;
  const int ns = s.nslot[rl];
  for (int t = tid; t < ns * SEL_BINS; t += 256) h[t] = 0;
  if (tid < SEL_MAXT) spre[tid] = s.slotpre[rl * SEL_MAXT + tid];
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const int64_t w = WEIGHTED ? (c0 + rl) / R_v : 0, v = WEIGHTED ? (c0 + rl) % R_v : c0 + rl;
  const double *row = V + v * row_stride;
  const int64_t base = c * slice, end = (base + slice < S) ? base + slice : S;
  bool seen_nan = false;
  for (int64_t off = base; off < end; off += 256) {   // the trip count is the same for every lane
    const int64_t i = off + tid;
    int bin = -1;
    u64 wt = 0;
    if (i < end) {
      const double x = row[i * elem_stride];
      const u64 key = sel_key(x);
      if (pass == 0) {
        bin = (int)(key >> 56);
        seen_nan |= (x != x);
      } else {
        const u64 hi = key >> (shift + 8);
        for (int j = 0; j < ns; ++j)
          if ((spre[j] >> (shift + 8)) == hi) bin = j * SEL_BINS + (int)((key >> shift) & 255);
      }
      if (WEIGHTED && bin >= 0) {
        wt = q[w * ldq + i];
        if (wt == 0) bin = -1;
      }
    }
    // the lanes that agree with the wave's first lane add once: the leading bytes of real data are nearly constant
    const int lead = __builtin_amdgcn_readfirstlane(bin);
    if (WEIGHTED) {
      const u64 led = wave_sum_u64(bin == lead ? wt : 0);
      if (lead >= 0 && lane == 0) atomicAdd(&h[lead], (bin_t)led);
      if (bin >= 0 && bin != lead) atomicAdd(&h[bin], (bin_t)wt);
    } else {
      const u64 same = __ballot(bin == lead);
      if (lead >= 0 && lane == 0) atomicAdd(&h[lead], (bin_t)__popcll(same));
      if (bin >= 0 && bin != lead) atomicAdd(&h[bin], (bin_t)1);
    }
  }
  __syncthreads();
  u64 *g = s.hist + rl * (SEL_MAXT * SEL_BINS);
  for (int t = tid; t < ns * SEL_BINS; t += 256)
    if (h[t]) atomicAdd(&g[t], (u64)h[t]);
  if (seen_nan) s.nan[rl] = 1;
}

// one workgroup per pair: extend every target's prefix by the digit of this pass, regroup the slots, clear the histograms
__global__ __launch_bounds__(256) void sel_scan_kernel(SelState s, int nt, int pass) {
  __shared__ u64 sh[SEL_MAXT * SEL_BINS];
  __shared__ u64 pre[SEL_MAXT];
  const int tid = threadIdx.x;
  const int64_t rl = blockIdx.x;
  const int ns = s.nslot[rl];
  u64 *g = s.hist + rl * (SEL_MAXT * SEL_BINS);
  for (int t = tid; t < ns * SEL_BINS; t += 256) {
    sh[t] = g[t];
    g[t] = 0;
  }
  __syncthreads();
  const int shift = 56 - 8 * pass;
  if (tid < nt) {
    const int64_t i = rl * SEL_MAXT + tid;
    const u64 *hs = sh + s.slot[i] * SEL_BINS;
    const u64 t = s.trem[i];
    u64 below = 0;
    int digit = -1;
    for (int b = 0; b < SEL_BINS; ++b) {
      const u64 wsum = hs[b];
      if (t <= below + wsum) { digit = b; break; }   // the first bin whose cumulative weight reaches the target
      below += wsum;
    }
    if (digit < 0) {   // above the total weight: no element answers
      s.over[i] = 1;
      digit = SEL_BINS - 1;
      below = t - 1;
    }
    const u64 p = s.prefix[i] | ((u64)digit << shift);
    s.prefix[i] = p;
    s.trem[i] = t - below;   // the target within the bin: in [1, wsum]
    pre[tid] = p;
  }
  __syncthreads();
  if (tid == 0) {   // sorted targets: prefixes ascend, equal ones are neighbours
    int n = 0;
    for (int r = 0; r < nt; ++r) {
      if (r == 0 || pre[r] != pre[r - 1]) s.slotpre[rl * SEL_MAXT + n++] = pre[r];
      s.slot[rl * SEL_MAXT + r] = n - 1;
    }
    s.nslot[rl] = n;
  }
}

// out[(c0 + rl) nt_all + perm[w][t]] = the element found; perm: [R_w][nt_all], of this group's targets
__global__ __launch_bounds__(256) void sel_out_kernel(SelState s, int rows, int nt, const int *__restrict__ perm,
                                                      int64_t nt_all, int64_t c0, int64_t R_v,
                                                      double *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * nt) return;
  const int rl = i / nt, t = i % nt;
  const int64_t w = (c0 + rl) / R_v;
  const bool bad = s.nan[rl] || s.over[rl * SEL_MAXT + t];
  out[(c0 + rl) * nt_all + perm[w * nt_all + t]] = bad ? sel_nan() : sel_value(s.prefix[rl * SEL_MAXT + t]);
}

int select_rows(const double *dV, int64_t R_v, int64_t S, int64_t row_stride, int64_t elem_stride, int64_t R_w,
                const u64 *dq, int64_t ldq, int64_t nt_all, const u64 *targets, double *dout, int64_t rows_cap,
                void (*on_pass)(), hipStream_t st) {
  const int64_t pairs = R_w * R_v;
  // per weight row: the targets ascending, and where each goes in the caller's order
  std::vector<u64> sorted((size_t)(R_w * nt_all));
  std::vector<int> perm((size_t)(R_w * nt_all));
  for (int64_t w = 0; w < R_w; ++w) {
    int *o = perm.data() + w * nt_all;
    const u64 *tw = targets + w * nt_all;
    std::iota(o, o + nt_all, 0);
    std::stable_sort(o, o + nt_all, [&](int x, int y) { return tw[x] < tw[y]; });
    for (int64_t i = 0; i < nt_all; ++i) sorted[(size_t)(w * nt_all + i)] = tw[o[i]];
  }
  DevScope sc(st);
  SelState s;
  u64 *dt = nullptr;
  int *dperm = nullptr;
  GP_TRY(sc.alloc(&s.prefix, rows_cap * SEL_MAXT));
  GP_TRY(sc.alloc(&s.trem, rows_cap * SEL_MAXT));
  GP_TRY(sc.alloc(&s.slotpre, rows_cap * SEL_MAXT));
  GP_TRY(sc.alloc(&s.slot, rows_cap * SEL_MAXT));
  GP_TRY(sc.alloc(&s.over, rows_cap * SEL_MAXT));
  GP_TRY(sc.alloc(&s.nslot, rows_cap));
  GP_TRY(sc.alloc(&s.nan, rows_cap));
  GP_TRY(sc.alloc(&s.hist, rows_cap * SEL_MAXT * SEL_BINS));
  GP_TRY(sc.alloc(&dt, R_w * nt_all));
  GP_TRY(sc.alloc(&dperm, R_w * nt_all));
  GP_TRY(upload(dt, sorted.data(), R_w * nt_all, st));
  GP_TRY(upload(dperm, perm.data(), R_w * nt_all, st));
  GP_HIP(hipMemsetAsync(s.hist, 0, sizeof(u64) * (size_t)rows_cap * SEL_MAXT * SEL_BINS, st));

  for (int64_t c0 = 0; c0 < pairs; c0 += rows_cap) {
    const int rows = (int)std::min<int64_t>(rows_cap, pairs - c0);
    // slices: at least SEL_SLICE elements, about SEL_MAX_WG workgroups per launch; whole multiples of the workgroup
    int64_t nblk = std::max<int64_t>(1, std::min((S + SEL_SLICE - 1) / SEL_SLICE, SEL_MAX_WG / rows));
    const int64_t slice = round_up((S + nblk - 1) / nblk, 256);
    nblk = (S + slice - 1) / slice;
    for (int64_t g0 = 0; g0 < nt_all; g0 += SEL_MAXT) {
      const int nt = (int)std::min<int64_t>(SEL_MAXT, nt_all - g0);
      hipLaunchKernelGGL(sel_init_kernel, dim3((unsigned)((rows * SEL_MAXT + 255) / 256)), dim3(256), 0, st, s, rows, nt,
                         dt + g0, nt_all, c0, R_v);
      GP_HIP(hipGetLastError());
      for (int pass = 0; pass < SEL_PASSES; ++pass) {
        on_pass();
        hipLaunchKernelGGL(dq ? sel_hist_kernel<true> : sel_hist_kernel<false>, dim3((unsigned)(rows * nblk)), dim3(256),
                           0, st, s, dV, row_stride, elem_stride, S, dq, ldq, c0, R_v, (int)nblk, slice, pass);
        GP_HIP(hipGetLastError());
        hipLaunchKernelGGL(sel_scan_kernel, dim3((unsigned)rows), dim3(256), 0, st, s, nt, pass);
        GP_HIP(hipGetLastError());
      }
      hipLaunchKernelGGL(sel_out_kernel, dim3((unsigned)((rows * nt + 255) / 256)), dim3(256), 0, st, s, rows, nt,
                         dperm + g0, nt_all, c0, R_v, dout);
      GP_HIP(hipGetLastError());
    }
  }
  GP_HIP(hipStreamSynchronize(st));   // `sorted` and `perm` are read by the copies above
  return GPEMU_OK;
}

}  // namespace gpemu
