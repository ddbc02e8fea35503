// Host check of the device-resource ledger (csrc/devledger.h), with made-up pointers and no GPU: see
// tests/test_devledger_host.py.  Prints "checks N failures M"; exits non-zero on a failure.
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../bayesian-inference_amd/csrc/devledger.h"

namespace gpemu {
DevLedger &dev_ledger() {   // the library defines its one ledger in gpemu_api.hip; this program has its own
  static DevLedger ledger;
  return ledger;
}
}  // namespace gpemu

using gpemu::DevLedger;

static int g_checks = 0, g_failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    ++g_checks;                                                         \
    if (!(cond)) {                                                      \
      ++g_failures;                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
    }                                                                   \
  } while (0)

static const void *fake(uintptr_t i) { return (const void *)(uintptr_t)(0x1000 + 256 * i); }

static bool balanced(const DevLedger::Stats &s) { return s.allocs - s.frees == s.live_blocks; }

// what DevScope does with the ledger: alloc notes, the destructor forgets what is still held, release hands a pointer on
struct Scope {
  DevLedger &L;
  std::vector<const void *> held;
  explicit Scope(DevLedger &l) : L(l) {}
  ~Scope() { for (const void *p : held) L.forget(p); }
  const void *alloc(uintptr_t i, size_t bytes) { L.note(fake(i), bytes); held.push_back(fake(i)); return fake(i); }
  const void *release(const void *p) {
    for (size_t i = 0; i < held.size(); ++i)
      if (held[i] == p) { held.erase(held.begin() + (std::ptrdiff_t)i); break; }
    return p;
  }
};

static void note_and_forget() {
  DevLedger L;
  DevLedger::Stats s = L.stats();
  CHECK(s.live_blocks == 0 && s.live_bytes == 0 && s.allocs == 0 && s.frees == 0 && s.live_streams == 0 && s.live_events == 0);
  L.note(fake(1), 100);
  L.note(fake(2), 28);
  s = L.stats();
  CHECK(s.live_blocks == 2 && s.live_bytes == 128 && s.allocs == 2 && s.frees == 0 && balanced(s));
  L.forget(fake(1));
  s = L.stats();
  CHECK(s.live_blocks == 1 && s.live_bytes == 28 && s.allocs == 2 && s.frees == 1 && balanced(s));
  // a free of null counts nothing; nor does a pointer the ledger never saw, or one already gone
  L.forget(nullptr);
  L.forget(fake(77));
  L.forget(fake(1));
  L.note(nullptr, 64);
  s = L.stats();
  CHECK(s.live_blocks == 1 && s.live_bytes == 28 && s.allocs == 2 && s.frees == 1 && balanced(s));
  // an address that comes back after its free is a new block
  L.note(fake(1), 8);
  s = L.stats();
  CHECK(s.live_blocks == 2 && s.live_bytes == 36 && s.allocs == 3 && balanced(s));
  L.forget(fake(1));
  L.forget(fake(2));
  s = L.stats();
  CHECK(s.live_blocks == 0 && s.live_bytes == 0 && s.allocs == 3 && s.frees == 3);
  // an address noted twice without a free between: the earlier block counts as gone, the books still balance
  L.note(fake(5), 16);
  L.note(fake(5), 48);
  s = L.stats();
  CHECK(s.live_blocks == 1 && s.live_bytes == 48 && balanced(s));
  L.forget(fake(5));
  s = L.stats();
  CHECK(s.live_blocks == 0 && s.live_bytes == 0 && balanced(s));
}

static void release_keeps_live() {
  DevLedger L;
  const void *kept = nullptr;
  {
    Scope sc(L);
    sc.alloc(1, 10);
    kept = sc.release(sc.alloc(2, 20));
    sc.alloc(3, 30);
    CHECK(L.stats().live_blocks == 3 && L.stats().live_bytes == 60);
  }
  DevLedger::Stats s = L.stats();
  CHECK(s.live_blocks == 1 && s.live_bytes == 20 && s.allocs == 3 && s.frees == 2 && balanced(s));
  L.forget(kept);
  s = L.stats();
  CHECK(s.live_blocks == 0 && s.live_bytes == 0 && balanced(s));
}

static void streams_and_events() {
  DevLedger L;
  L.stream_made(); L.stream_made(); L.event_made();
  CHECK(L.stats().live_streams == 2 && L.stats().live_events == 1);
  L.stream_gone(); L.event_gone();
  CHECK(L.stats().live_streams == 1 && L.stats().live_events == 0);
  L.stream_gone();
  CHECK(L.stats().live_streams == 0 && L.stats().live_blocks == 0);
}

static void refusal() {
  DevLedger L;
  CHECK(!L.armed());
  CHECK(!L.refuse_now());                    // never armed: nothing is refused
  CHECK(!L.arm(3));                          // nothing was armed before
  CHECK(L.armed());
  CHECK(!L.refuse_now());
  CHECK(!L.refuse_now());
  CHECK(L.armed());
  CHECK(L.refuse_now());                     // the third
  CHECK(!L.armed());                         // disarmed by firing
  for (int i = 0; i < 5; ++i) CHECK(!L.refuse_now());
  CHECK(!L.arm(0));                          // it had fired: not still armed
  CHECK(!L.arm(1));
  CHECK(L.refuse_now());                     // nth = 1: the very next
  CHECK(!L.refuse_now());
  CHECK(!L.arm(2));
  CHECK(!L.refuse_now());
  CHECK(L.arm(0));                           // disarmed before it fired: reported as still armed
  CHECK(!L.armed());
  CHECK(!L.refuse_now());
  CHECK(!L.refuse_now());
  CHECK(!L.arm(5));
  CHECK(L.arm(2));                           // re-armed over a pending one: reported, and the new count holds
  CHECK(!L.refuse_now());
  CHECK(L.refuse_now());
  CHECK(!L.arm(-4));                         // not positive: disarmed
  CHECK(!L.armed());
  // a refused allocation is never noted: the caller returns before the allocator, so the books do not move
  DevLedger::Stats s = L.stats();
  CHECK(s.allocs == 0 && s.live_blocks == 0);
}

static void threads() {
  DevLedger L;
  constexpr int T = 8, PER = 10000;
  L.arm((int64_t)T * PER / 2);               // fires exactly once, in whichever thread makes that allocation
  std::vector<int> fired(T, 0);
  std::vector<std::thread> pool;
  for (int t = 0; t < T; ++t)
    pool.emplace_back([&L, &fired, t]() {
      for (int i = 0; i < PER; ++i) {
        const void *p = fake((uintptr_t)t * PER + (uintptr_t)i + 1);
        if (L.refuse_now()) ++fired[t];      // refused: never noted, and its later free counts nothing
        else L.note(p, 8 + (size_t)(i % 5));
        if (i % 3 == 0) { L.stream_made(); L.stream_gone(); }
        if (i >= 4) L.forget(fake((uintptr_t)t * PER + (uintptr_t)(i - 4) + 1));   // four in flight per thread
      }
      for (int i = PER - 4; i < PER; ++i) L.forget(fake((uintptr_t)t * PER + (uintptr_t)i + 1));
    });
  for (std::thread &th : pool) th.join();
  int total = 0;
  for (int f : fired) total += f;
  const DevLedger::Stats s = L.stats();
  CHECK(total == 1);
  CHECK(!L.armed());
  CHECK(s.live_blocks == 0 && s.live_bytes == 0 && s.live_streams == 0);
  CHECK(s.allocs == (int64_t)T * PER - 1 && s.frees == s.allocs);
}

int main() {
  note_and_forget();
  release_keeps_live();
  streams_and_events();
  refusal();
  threads();
  CHECK(&gpemu::dev_ledger() == &gpemu::dev_ledger());
  std::printf("checks %d failures %d\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
