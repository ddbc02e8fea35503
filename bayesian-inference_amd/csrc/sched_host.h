// Host side of the large-batch triangular GEMM and of the cross-kernel that feeds it (k_predict.hip): the item type and
// the LPT schedule of one launch shape, the cross-kernel's workgroup -> unit map, and the tables of the sampler's
// compacted half-step (one schedule and one map per live block count).  Nothing here touches the device or a model
// handle: k_predict.hip wraps these builders with the caching and the upload, and tests/native/sched_host_check.cpp
// compiles this header alone with g++ and checks every table it produces.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define GPEMU_SCHED_HD __host__ __device__
#else
#define GPEMU_SCHED_HD
#endif

namespace gpemu {

constexpr int TM = 64;      // rows per item
constexpr int KT = 32;      // K step
struct TrmmItem {
  int p, rb, col0, half;  // PC, 64-row block, first column, 1 = 64-column item
};
constexpr int TRMM_MAX_ITEMS = 64;  // per worker; the schedule falls back to more workers' worth otherwise
constexpr int SCHED_TILE = 128;        // column tile of the triangular GEMM (internal.h: TILE)
constexpr int SCHED_KSTAR_ROWS = 64;   // training rows per workgroup of the large-batch cross-kernel (internal.h: KSTAR_ROWS_BIG)

// what the builders need to know of a model: PCs, 64-row blocks of the triangular GEMM, padded training rows, CUs
struct SchedShape {
  int k, nrb;
  int64_t Npad;
  int num_cu;
};

// the (PC, row chunk, 64-column block) of workgroup bidx in the grid of a whole batch
struct KstarUnit { int p, chunk, cb; };
GPEMU_SCHED_HD static inline KstarUnit kstar_unit(int bidx, int nchunk, int ncb64, int gper, int ncbp) {
  KstarUnit u;
  if (gper > 0) {
    // the GEMM runs one launch per piece of ncbp 128-column blocks (launch_trmm_vsq: at most 512 columns each), every
    // launch dealing its k ncbp groups to the XCDs in (PC, column block) order, gper per XCD
    const int xcd = bidx & 7, slot = bidx >> 3;
    const int half = slot & 1, rest = slot >> 1;
    u.chunk = rest % nchunk;
    const int rest2 = rest / nchunk;
    const int piece = rest2 / gper, g = xcd * gper + rest2 % gper;
    u.p = g / ncbp;
    u.cb = 2 * (piece * ncbp + g % ncbp) + half;
  } else {
    u.cb = bidx % ncb64;
    const int rest = bidx / ncb64;
    u.chunk = rest % nchunk;
    u.p = rest / nchunk;
  }
  return u;
}
// a unit as an entry of KstarArgs::kmap: p < 64, chunk < 4096, cb < 256
GPEMU_SCHED_HD static inline int kstar_pack(const KstarUnit &u) { return (u.p << 20) | (u.chunk << 8) | u.cb; }

// LPT schedule of the items of one launch shape (cached per model and column-tile count)
// keep (probes only, tools/share_probe.hip): restrict the launch to the (PC, 64-row block) pairs it accepts
// live64 >= 0 (the sampler's compacted half-step, build_live_tables below): only the first live64 64-column blocks hold
// queries.  The 128-column blocks beyond them get no items, and an odd count leaves the last one half filled: all its row
// blocks are then 64-column items of its left half.  The grid is that of the whole batch (workers), whatever is left to
// do; form: where the items go (internal.h: LiveCols).  live64 < 0 is the whole batch, as ever.
static inline void build_trmm_schedule(const SchedShape &s, int ncb, std::vector<TrmmItem> &flat, std::vector<int> &cnt,
                                       int &max_items, int &nworkers, bool (*keep)(int p, int rb) = nullptr,
                                       int split_all = 0, int live64 = -1, int form = 1, int workers = 0) {
  constexpr int TILE = SCHED_TILE;
  const int nrb = s.nrb, k = s.k;
  struct It { double cost; TrmmItem it; int xcd; };
  std::vector<It> items;
  // row blocks with short K are issued as two 64-column halves; with one or two column blocks (B <= 256) there
  // are too few items for 256 workers unless every row block is
  int split_below = (ncb <= 2 || split_all) ? nrb : nrb / 4;
  if (live64 >= 0 && workers > 0 && split_below < nrb) {
    // few live blocks: once the longest 128-column item outweighs a worker's share of the whole launch, it alone sets
    // the launch's time (N = 1000, 10 PCs: 72 us from 2 to 5 of 8 blocks; at 5 the halved items are no faster) -- halve every item then, as at ncb <= 2
    double total = 0.0;
    for (int rb = 0; rb < nrb; ++rb) total += 0.5 * k * std::min(live64, 2 * ncb) * (double)(((int64_t)rb * TM + TM + KT - 1) / KT);
    const double top = (double)(((int64_t)(nrb - 1) * TM + TM + KT - 1) / KT);
    if (top > 1.3 * total / workers) split_below = nrb;
  }
  // per-item cost of the epilogue, in k-tiles.  Measured (in-kernel stamps, profiles/r03_trmm_balance.txt): workers with
  // 2 / 3 / 5 items finish at 85.3 / 87.6 / 88.5 us, but raising it to 0.4-0.9 (3 / 4 items everywhere) leaves the slowest
  // worker at 91 us: the spread is the XCDs' (means 86.6-88.2 us), not the cost model's
  const double ov = 0.15;
  for (int rb = 0; rb < nrb; ++rb) {
    const double nt = (double)(((int64_t)rb * TM + TM + KT - 1) / KT);
    for (int p = 0; p < k; ++p)
      for (int cb = 0; cb < ncb; ++cb) {
        if (keep && !keep(p, rb)) continue;
        const int halves = live64 < 0 ? 2 : std::min(2, std::max(0, live64 - 2 * cb));   // live halves of this block
        if (halves == 0) continue;
        if (rb < split_below || halves == 1) {
          items.push_back({0.5 * nt + ov, TrmmItem{p, rb, cb * TILE, 1}, 0});
          if (halves == 2) items.push_back({0.5 * nt + ov, TrmmItem{p, rb, cb * TILE + 64, 1}, 0});
        } else {
          items.push_back({nt + ov, TrmmItem{p, rb, cb * TILE, 0}, 0});
        }
      }
  }
  const int ncu = s.num_cu;
  nworkers = workers > 0 ? workers : (ncu < (int)items.size() ? ncu : (int)items.size());
  const int nxcd = 8, ngroups = k * ncb;
  const bool by_xcd = !keep && nworkers == ncu && nworkers % nxcd == 0;
  const bool by_cost = by_xcd && live64 >= 0 && form == 2;
  if (by_cost) {
    // Fewer live blocks than the batch has: the groups that are left no longer divide evenly over the XCDs, and a half
    // filled block costs half.  The items in (PC, column block, row block) order are cut at eighths of the total cost:
    // an XCD still works on neighbouring groups, and a group that straddles a cut has its row blocks divided between
    // two neighbouring XCDs (the cross-kernel's workgroups follow the same order: build_live_tables)
    std::vector<int> ord(items.size());
    for (size_t i = 0; i < ord.size(); ++i) ord[i] = (int)i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
      const TrmmItem &x = items[a].it, &y = items[b].it;
      if (x.p != y.p) return x.p < y.p;
      if (x.col0 / TILE != y.col0 / TILE) return x.col0 / TILE < y.col0 / TILE;
      if (x.rb != y.rb) return x.rb < y.rb;
      return x.col0 < y.col0;
    });
    double total = 0.0, run = 0.0;
    for (const It &x : items) total += x.cost;
    for (int i : ord) {
      const int xcd = (int)((run + 0.5 * items[i].cost) * nxcd / total);
      items[i].xcd = xcd < 0 ? 0 : (xcd > nxcd - 1 ? nxcd - 1 : xcd);
      run += items[i].cost;
    }
  }
  std::stable_sort(items.begin(), items.end(), [](const It &a, const It &b) { return a.cost > b.cost; });
  std::vector<std::vector<TrmmItem>> per(nworkers);
  std::vector<double> load(nworkers, 0.0);
  // XCD-aware placement.  Workgroups are dispatched round-robin over the 8 XCDs (worker w runs on XCD w % 8),
  // each with its own 4 MiB L2.  All items of one (PC, column block) group read the same K_*^T block and the
  // groups of one PC read the same W_p; every group costs the same, so when the groups divide evenly they are
  // dealt to the XCDs in (PC, column block) order -- an XCD then works on at most two or three PCs, and the
  // column-block items of one (PC, row block), equally long, start together and stream the same W rows through
  // that L2 -- and LPT runs within each XCD's workers.  Otherwise: plain LPT over all workers.
  if (by_cost || (by_xcd && ngroups % nxcd == 0)) {
    const int gper = ngroups / nxcd;
    for (const It &x : items) {
      const int g = x.it.p * ncb + x.it.col0 / TILE;
      const int xcd = by_cost ? x.xcd : g / gper;
      int best = xcd;
      for (int w = xcd; w < nworkers; w += nxcd)
        if (load[w] < load[best]) best = w;
      per[best].push_back(x.it);
      load[best] += x.cost;
    }
  } else {
    for (const It &x : items) {  // longest processing time first onto the least loaded worker
      int best = 0;
      for (int w = 1; w < nworkers; ++w)
        if (load[w] < load[best]) best = w;
      per[best].push_back(x.it);
      load[best] += x.cost;
    }
  }
  max_items = 1;
  for (auto &v : per) max_items = v.size() > (size_t)max_items ? (int)v.size() : max_items;
  flat.assign((size_t)nworkers * max_items, TrmmItem{0, 0, 0, 0});
  cnt.assign(nworkers, 0);
  for (int w = 0; w < nworkers; ++w) {
    cnt[w] = (int)per[w].size();
    for (size_t i = 0; i < per[w].size(); ++i) flat[(size_t)w * max_items + i] = per[w][i];
  }
}

// How the live blocks of a count are dealt where nothing else is asked for (LiveCols::form < 0): measured per count at
// N = 1000, 10 PCs, 512 columns (tools/time_compact.py, profiles/compact_forms.txt)
static inline int live_default_form(int live64, int ncb64) {
  (void)live64; (void)ncb64;
  return 2;
}

// The compacted half-step's tables for batches of ncb 128-column blocks: for every live count c = 0 .. 2 ncb the GEMM's
// schedule (row c of items / cnt, all with the workers and the item stride of the widest) and the cross-kernel's
// workgroup -> unit map (row c of kmap).  Row 2 ncb is the whole batch's own schedule and map, item for item.
struct LiveTables {
  std::vector<TrmmItem> items;   // [2 ncb + 1][workers][stride]
  std::vector<int> cnt;          // [2 ncb + 1][workers]
  std::vector<int> kmap;         // [2 ncb + 1][nwg]: kstar_pack of the workgroup's unit, or -1
  std::vector<int> forms;        // [2 ncb + 1]: the form each row was built in (row 2 ncb: 0, the whole batch)
  std::vector<int> fell;         // [2 ncb + 1]: LIVE_FELL_* bits of the fallbacks the row took
  int stride = 0, workers = 0, nwg = 0;
  int full_max_items = 0;        // items per worker of the whole batch's schedule (what LIVE_TABLES_TOO_MANY_ITEMS is about)
};
enum { LIVE_FELL_TO_1 = 1, LIVE_FELL_TO_0 = 2 };
enum { LIVE_TABLES_OK = 0, LIVE_TABLES_NO_MAP = 1, LIVE_TABLES_TOO_MANY_ITEMS = 2 };

// form: LiveCols::form (< 0: live_default_form per count).  LIVE_TABLES_NO_MAP: the shape does not fit kstar_pack;
// LIVE_TABLES_TOO_MANY_ITEMS: the whole batch's schedule does not fit a worker's list (out.full_max_items).
static inline int build_live_tables(const SchedShape &s, int ncb, int form, LiveTables &out) {
  const int cap = s.num_cu;
  const int k = s.k, ncb64 = 2 * ncb, nchunk = (int)(s.Npad / SCHED_KSTAR_ROWS), nwg = ncb64 * nchunk * k;
  out.nwg = nwg;
  if (k > 64 || nchunk > 4096 || ncb64 > 255) return LIVE_TABLES_NO_MAP;
  std::vector<std::vector<TrmmItem>> flats(ncb64 + 1);
  std::vector<std::vector<int>> cnts(ncb64 + 1);
  std::vector<int> mx(ncb64 + 1, 1);
  out.forms.assign(ncb64 + 1, 0);
  out.fell.assign(ncb64 + 1, 0);
  std::vector<int> &forms = out.forms;
  int workers = 0;
  build_trmm_schedule(s, ncb, flats[ncb64], cnts[ncb64], mx[ncb64], workers);
  out.full_max_items = mx[ncb64];
  if (mx[ncb64] > TRMM_MAX_ITEMS) return LIVE_TABLES_TOO_MANY_ITEMS;
  const int ngroups = k * ncb;
  const bool by_xcd = workers == cap && cap % 8 == 0;
  // the whole batch's map (kstar_setup, one piece)
  const int gper = (ngroups % 8 == 0 && cap % 8 == 0) ? ngroups / 8 : 0;
  int stride = mx[ncb64];
  for (int c = 0; c < ncb64; ++c) {
    int f = form >= 0 ? form : live_default_form(c, ncb64);
    const int units = k * c * nchunk;                       // the cross-kernel's workgroups with work
    // by cost only where every CU is a GEMM worker and the eighths of the units fit the cross-kernel's grid
    if (f == 2 && (!by_xcd || (units + 7) / 8 * 8 > nwg)) { f = 1; out.fell[c] |= LIVE_FELL_TO_1; }
    if (f != 0) {
      int nw = 0;
      build_trmm_schedule(s, ncb, flats[c], cnts[c], mx[c], nw, nullptr, 0, c, f, workers);
      // a count's own deal can need more items per worker than the whole batch's (every item halved): the whole
      // batch's schedule then, whose items beyond the live blocks the kernel skips
      if (mx[c] > TRMM_MAX_ITEMS) { f = 0; out.fell[c] |= LIVE_FELL_TO_0; }
    }
    if (f == 0) { flats[c] = flats[ncb64]; cnts[c] = cnts[ncb64]; mx[c] = mx[ncb64]; }
    forms[c] = f;
    stride = std::max(stride, mx[c]);
  }
  out.items.assign((size_t)(ncb64 + 1) * workers * stride, TrmmItem{0, 0, 0, 0});
  out.cnt.assign((size_t)(ncb64 + 1) * workers, 0);
  out.kmap.assign((size_t)(ncb64 + 1) * nwg, -1);
  for (int c = 0; c <= ncb64; ++c) {
    for (int w = 0; w < workers; ++w) {
      out.cnt[(size_t)c * workers + w] = cnts[c][w];
      for (int i = 0; i < cnts[c][w]; ++i)
        out.items[((size_t)c * workers + w) * stride + i] = flats[c][(size_t)w * mx[c] + i];
    }
    int *row = out.kmap.data() + (size_t)c * nwg;
    if (forms[c] == 2) {
      // the units in (PC, 128-column block, row chunk, half) order, an eighth of them to each XCD (workgroup i runs on
      // XCD i % 8), in that order: the GEMM's cuts, to within the group that straddles one
      std::vector<int> list;
      for (int p = 0; p < k; ++p)
        for (int cb = 0; cb < ncb; ++cb)
          for (int ch = 0; ch < nchunk; ++ch)
            for (int h = 0; h < 2; ++h)
              if (2 * cb + h < c) list.push_back(kstar_pack(KstarUnit{p, ch, 2 * cb + h}));
      const int n = (int)list.size(), per = (n + 7) / 8;
      for (int i = 0; i < n; ++i) row[(i % per) * 8 + i / per] = list[i];
    } else {
      for (int i = 0; i < nwg; ++i) {
        const KstarUnit u = kstar_unit(i, nchunk, ncb64, gper, ncb);
        if (u.cb < c) row[i] = kstar_pack(u);
      }
    }
  }
  out.stride = stride;
  out.workers = workers;
  return LIVE_TABLES_OK;
}

}  // namespace gpemu
