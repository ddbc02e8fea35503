// Host-side check of the triangular GEMM's schedules and of the compacted half-step's tables
// (bayesian-inference_amd/csrc/sched_host.h), built with g++ by tests/test_sched_host.py.  For every shape of a sweep over
// PCs, padded training rows, 128-column blocks, CUs and forms, and every live block count c = 0 .. 2 ncb of it:
//   cover      the items of row c, expanded into 64-column cells, are exactly (PC, row block, cell < c') once each
//              (c' = c, or 2 ncb where the row is the whole batch's schedule: form 0)
//   fields     col0 on a 64-column boundary, on a 128-column one for a full item; every list within TRMM_MAX_ITEMS and the
//              stride; nothing but zeros behind a list
//   kmap       the entries >= 0 of row c, decoded as the cross-kernel does, are exactly (PC, row chunk, cb < c) once each
//   full row   row 2 ncb is build_trmm_schedule(ncb) item for item, and kstar_unit(i) for every workgroup i
//   stable     a second call builds the same tables
// A dropped item leaves a stale partial sum and a doubled one only wastes time: neither can be seen by comparing two
// forms of the library on a few shapes, both are counted here.
//   usage: sched_host_check [every]     (every: take each every-th shape of the sweep, default 1)
// prints the number of rows built in each form and through each fallback, and "failures N"; exit status 1 if N > 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bayesian-inference_amd/csrc/sched_host.h"

using namespace gpemu;

static long g_fail = 0;
#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      if (++g_fail <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                                       \
  } while (0)

// every (PC, row block, 64-column cell < ncell) with keep(p, rb) exactly once in the lists of one schedule
static void check_schedule(const SchedShape &s, const TrmmItem *items, const int *cnt, int workers, int stride, int ncell,
                           bool (*keep)(int, int), const char *what, int c) {
  std::vector<unsigned char> seen((size_t)s.k * s.nrb * (ncell > 0 ? ncell : 1), 0);
  long cells = 0;
  for (int w = 0; w < workers; ++w) {
    CHECK(cnt[w] >= 0 && cnt[w] <= TRMM_MAX_ITEMS && cnt[w] <= stride, "%s c %d worker %d cnt %d stride %d", what, c, w, cnt[w], stride);
    for (int i = 0; i < stride; ++i) {
      const TrmmItem &it = items[(size_t)w * stride + i];
      if (i >= cnt[w]) {
        CHECK(it.p == 0 && it.rb == 0 && it.col0 == 0 && it.half == 0, "%s c %d worker %d: entry %d behind the list is not zero", what, c, w, i);
        continue;
      }
      CHECK(it.half == 0 || it.half == 1, "%s c %d half %d", what, c, it.half);
      CHECK(it.col0 >= 0 && it.col0 % 64 == 0, "%s c %d col0 %d", what, c, it.col0);
      CHECK(it.half != 0 || it.col0 % 128 == 0, "%s c %d full item at col0 %d", what, c, it.col0);
      CHECK(it.p >= 0 && it.p < s.k && it.rb >= 0 && it.rb < s.nrb, "%s c %d item (%d, %d)", what, c, it.p, it.rb);
      if (it.p < 0 || it.p >= s.k || it.rb < 0 || it.rb >= s.nrb || it.col0 < 0) continue;
      for (int h = 0; h < (it.half ? 1 : 2); ++h) {
        const int cell = it.col0 / 64 + h;
        CHECK(cell < ncell, "%s c %d: item (%d, %d, col0 %d, half %d) beyond the %d live cells", what, c, it.p, it.rb, it.col0, it.half, ncell);
        if (cell >= ncell) continue;
        unsigned char &f = seen[((size_t)it.p * s.nrb + it.rb) * ncell + cell];
        CHECK(f == 0, "%s c %d: cell (%d, %d, %d) twice", what, c, it.p, it.rb, cell);
        f = 1;
        ++cells;
      }
    }
  }
  long want = 0;
  for (int p = 0; p < s.k; ++p)
    for (int rb = 0; rb < s.nrb; ++rb) {
      const bool k = !keep || keep(p, rb);
      if (k) want += ncell;
      for (int cell = 0; cell < ncell; ++cell)
        if (seen[((size_t)p * s.nrb + rb) * ncell + cell] != (k ? 1 : 0)) {
          CHECK(false, "%s c %d: cell (%d, %d, %d) %s", what, c, p, rb, cell, k ? "missing" : "not kept, yet scheduled");
          break;
        }
    }
  CHECK(cells == want, "%s c %d: %ld cells, want %ld", what, c, cells, want);
}

// the entries >= 0 of one kmap row, decoded as kstar_body decodes them: every (PC, row chunk, cb < c) exactly once
static void check_kmap_row(const SchedShape &s, const int *row, int nwg, int nchunk, int c) {
  std::vector<unsigned char> seen((size_t)s.k * nchunk * (c > 0 ? c : 1), 0);
  long units = 0;
  for (int i = 0; i < nwg; ++i) {
    const int e = row[i];
    if (e < 0) { CHECK(e == -1, "kmap c %d entry %d = %d", c, i, e); continue; }
    const int p = e >> 20, chunk = (e >> 8) & 0xfff, cb = e & 0xff;
    CHECK(p < s.k && chunk < nchunk && cb < c, "kmap c %d entry %d: unit (%d, %d, %d)", c, i, p, chunk, cb);
    if (!(p < s.k && chunk < nchunk && cb < c)) continue;
    unsigned char &f = seen[((size_t)p * nchunk + chunk) * c + cb];
    CHECK(f == 0, "kmap c %d: unit (%d, %d, %d) twice", c, p, chunk, cb);
    f = 1;
    ++units;
  }
  CHECK(units == (long)s.k * nchunk * c, "kmap c %d: %ld units, want %ld", c, units, (long)s.k * nchunk * c);
}

static bool keep_checker(int p, int rb) { return (p + rb) % 2 == 0; }

struct Tally { long shapes = 0, accepted = 0, declined = 0, rows = 0, form[3] = {0, 0, 0}, fell1 = 0, fell0 = 0; };

// one shape in one form; returns false if the shape is declined
static bool check_shape(const SchedShape &s, int ncb, int form, Tally &t, bool twice) {
  LiveTables a;
  const int rc = build_live_tables(s, ncb, form, a);
  if (rc != LIVE_TABLES_OK) {
    CHECK(rc == LIVE_TABLES_TOO_MANY_ITEMS && a.full_max_items > TRMM_MAX_ITEMS, "k %d Npad %lld ncb %d cu %d: declined with %d (%d items)",
          s.k, (long long)s.Npad, ncb, s.num_cu, rc, a.full_max_items);
    return false;
  }
  const int ncb64 = 2 * ncb, nchunk = (int)(s.Npad / SCHED_KSTAR_ROWS);
  CHECK(a.nwg == ncb64 * nchunk * s.k, "nwg %d", a.nwg);
  CHECK(a.workers > 0 && a.workers <= s.num_cu && a.stride >= 1 && a.stride <= TRMM_MAX_ITEMS, "workers %d stride %d", a.workers, a.stride);
  CHECK((int)a.forms.size() == ncb64 + 1 && a.items.size() == (size_t)(ncb64 + 1) * a.workers * a.stride &&
        a.cnt.size() == (size_t)(ncb64 + 1) * a.workers && a.kmap.size() == (size_t)(ncb64 + 1) * a.nwg, "table sizes");
  if (g_fail) return true;
  for (int c = 0; c <= ncb64; ++c) {
    const int f = a.forms[c];
    CHECK(f >= 0 && f <= 2 && (form < 0 || c == ncb64 || f == form || a.fell[c]), "c %d: form %d asked %d", c, f, form);
    check_schedule(s, a.items.data() + (size_t)c * a.workers * a.stride, a.cnt.data() + (size_t)c * a.workers, a.workers, a.stride,
                   f == 0 ? ncb64 : c, nullptr, "live", c);
    check_kmap_row(s, a.kmap.data() + (size_t)c * a.nwg, a.nwg, nchunk, c);
    if (c < ncb64) {
      ++t.rows;
      ++t.form[f < 0 || f > 2 ? 0 : f];
      if (a.fell[c] & LIVE_FELL_TO_1) ++t.fell1;
      if (a.fell[c] & LIVE_FELL_TO_0) ++t.fell0;
    }
  }
  // the full row: the whole batch's own schedule, item for item, and the whole batch's own workgroup order
  std::vector<TrmmItem> flat;
  std::vector<int> cnt;
  int mx = 0, nw = 0;
  build_trmm_schedule(s, ncb, flat, cnt, mx, nw);
  CHECK(nw == a.workers && mx <= a.stride, "full row: %d workers (%d), %d items (stride %d)", nw, a.workers, mx, a.stride);
  if (nw == a.workers && mx <= a.stride)
    for (int w = 0; w < nw; ++w) {
      CHECK(cnt[w] == a.cnt[(size_t)ncb64 * a.workers + w], "full row: worker %d cnt", w);
      for (int i = 0; i < cnt[w] && i < a.stride; ++i)
        CHECK(memcmp(&flat[(size_t)w * mx + i], &a.items[((size_t)ncb64 * a.workers + w) * a.stride + i], sizeof(TrmmItem)) == 0,
              "full row: worker %d item %d", w, i);
    }
  // (kstar_setup's placement of one piece: whole groups per XCD where they divide evenly)
  const int ngroups = s.k * ncb, gper = (ngroups % 8 == 0 && s.num_cu % 8 == 0) ? ngroups / 8 : 0;
  for (int i = 0; i < a.nwg; ++i)
    CHECK(a.kmap[(size_t)ncb64 * a.nwg + i] == kstar_pack(kstar_unit(i, nchunk, ncb64, gper, ncb)), "full row: kmap entry %d", i);
  if (!twice) return true;
  // a second call
  LiveTables b;
  CHECK(build_live_tables(s, ncb, form, b) == LIVE_TABLES_OK, "second call declined");
  CHECK(b.forms == a.forms && b.workers == a.workers && b.stride == a.stride && b.nwg == a.nwg, "second call: forms / workers / stride");
  CHECK(b.cnt == a.cnt && b.kmap == a.kmap && b.items.size() == a.items.size() &&
        memcmp(b.items.data(), a.items.data(), sizeof(TrmmItem) * a.items.size()) == 0, "second call: tables");
  return true;
}

// the probes' parameters of the plain builder: every item halved, and a launch restricted to some (PC, row block) pairs
static void check_probe_parameters(const SchedShape &s, int ncb) {
  std::vector<TrmmItem> flat;
  std::vector<int> cnt;
  int mx = 0, nw = 0;
  build_trmm_schedule(s, ncb, flat, cnt, mx, nw, nullptr, 1);
  if (mx <= TRMM_MAX_ITEMS) {
    check_schedule(s, flat.data(), cnt.data(), nw, mx, 2 * ncb, nullptr, "split_all", 2 * ncb);
    for (const TrmmItem &it : flat) CHECK(it.half == 1 || (it.p == 0 && it.rb == 0 && it.col0 == 0), "split_all: a full item");
  }
  build_trmm_schedule(s, ncb, flat, cnt, mx, nw, keep_checker, 0);
  if (mx <= TRMM_MAX_ITEMS && nw > 0) check_schedule(s, flat.data(), cnt.data(), nw, mx, 2 * ncb, keep_checker, "keep", 2 * ncb);
}

int main(int argc, char **argv) {
  const int every = argc > 1 ? atoi(argv[1]) : 1;
  const int ks[] = {1, 2, 3, 10, 17, 40, 64}, npads[] = {128, 256, 384, 1024, 2048, 5120}, cus[] = {8, 64, 104, 256, 304};
  const int forms[] = {-1, 0, 1, 2};
  Tally t;
  long idx = 0, nheavy = 0;
  for (int k : ks)
    for (int Npad : npads)
      for (int ncb = 2; ncb <= 16; ++ncb)
        for (int cu : cus) {
          if (idx++ % every) continue;
          const SchedShape s{k, Npad / TM, Npad, cu};
          // Building the tables of a shape costs about (items of a row) x (rows) x (workers scanned per item).  Above
          // 10^6 of these the sweep is thinned to stay within seconds: every other such shape, in one of the four forms
          // (taken in turn), built once; the shapes below it, 60 % of the sweep, go through all four forms, built twice
          const double work = (double)k * s.nrb * ncb * (2 * ncb + 1) * cu;
          const bool heavy = work > 1.0e6;
          if (heavy && nheavy++ % 2) continue;
          ++t.shapes;
          bool ok = true;
          if (heavy) {
            const long h = nheavy - 1;
            ok = check_shape(s, ncb, forms[(h / 2) % 4], t, false);
          } else {
            for (int form : forms) {
              ok = check_shape(s, ncb, form, t, true);
              if (!ok) break;                                // (declined whatever the form: the whole batch's schedule)
            }
          }
          if (ok) { ++t.accepted; if (!heavy) check_probe_parameters(s, ncb); }
          else ++t.declined;
        }
  // the map's limits: 64 PCs, 4096 row chunks, 255 column blocks
  {
    LiveTables a;
    CHECK(build_live_tables(SchedShape{65, 2, 128, 256}, 2, -1, a) == LIVE_TABLES_NO_MAP, "k = 65 accepted");
    CHECK(build_live_tables(SchedShape{1, 2, 128, 256}, 128, -1, a) == LIVE_TABLES_NO_MAP, "ncb64 = 256 accepted");
    CHECK(build_live_tables(SchedShape{1, 4097, 4097 * 64, 256}, 2, -1, a) == LIVE_TABLES_NO_MAP, "nchunk = 4097 accepted");
    const KstarUnit u{63, 4095, 253};
    const int e = kstar_pack(u);
    CHECK(e >= 0 && (e >> 20) == 63 && ((e >> 8) & 0xfff) == 4095 && (e & 0xff) == 253, "pack round trip: %d", e);
  }
  printf("shapes %ld accepted %ld declined %ld rows %ld\n", t.shapes, t.accepted, t.declined, t.rows);
  printf("rows_form0 %ld rows_form1 %ld rows_form2 %ld fell_2_to_1 %ld fell_to_0 %ld\n", t.form[0], t.form[1], t.form[2], t.fell1, t.fell0);
  printf("failures %ld\n", g_fail);
  return g_fail ? 1 : 0;
}
