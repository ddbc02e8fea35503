// The ledger of the library's device resources: what devmem.h allocates and frees, and the streams and events the
// handles create.  Host bookkeeping only -- nothing of the HIP runtime is included or called here, so the header builds
// and is tested without a GPU (tests/native/devledger_check.cpp).  One object for the whole library, defined in
// gpemu_api.hip (dev_ledger()); any host thread may feed it.
//   Counted: every block of devmem.h (dev_alloc_bytes, dev_alloc_uncached, dev_free, ~DevScope, dev_reserve), by pointer
// and bytes asked for; streams and events made through stream_create / event_create (devmem.h).
//   Not counted: the IPC handles and mapped peer buffers of the walker-sharded transport, and whatever RCCL allocates for
// itself -- neither is memory the library owns.
//   The one-shot refusal ("the n-th allocation from now fails") is decided here, before the allocator is called: a test
// hook (gpemu_devmem_refuse_nth) that makes every early return of an allocation reachable without exhausting a device.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <unordered_map>

namespace gpemu {

class DevLedger {
 public:
  struct Stats { int64_t live_blocks, live_bytes, allocs, frees, live_streams, live_events; };

  // a block now exists (null: nothing to count)
  void note(const void *p, size_t bytes) {
    if (!p) return;
    std::lock_guard<std::mutex> lock(mu_);
    auto it = live_.find(p);
    if (it != live_.end()) {   // an address cannot be live twice: the earlier block went by without the ledger
      live_bytes_ -= (int64_t)it->second;
      ++frees_;
      it->second = bytes;
    } else {
      live_.emplace(p, bytes);
    }
    live_bytes_ += (int64_t)bytes;
    ++allocs_;
  }
  // a block is gone.  Null, or a pointer the ledger never saw (adopted from elsewhere), counts nothing.
  void forget(const void *p) {
    if (!p) return;
    std::lock_guard<std::mutex> lock(mu_);
    auto it = live_.find(p);
    if (it == live_.end()) return;
    live_bytes_ -= (int64_t)it->second;
    live_.erase(it);
    ++frees_;
  }
  void stream_made() { streams_.fetch_add(1, std::memory_order_relaxed); }
  void stream_gone() { streams_.fetch_sub(1, std::memory_order_relaxed); }
  void event_made() { events_.fetch_add(1, std::memory_order_relaxed); }
  void event_gone() { events_.fetch_sub(1, std::memory_order_relaxed); }

  // nth >= 1: the nth allocation from now is refused; 0: disarmed.  Returns whether an earlier arming had not fired.
  bool arm(int64_t nth) {
    std::lock_guard<std::mutex> lock(mu_);
    return refuse_in_.exchange(nth > 0 ? nth : 0, std::memory_order_relaxed) > 0;
  }
  bool armed() const { return refuse_in_.load(std::memory_order_relaxed) > 0; }
  // asked once per allocation, before the allocator: true exactly once, for the allocation that was armed, and the
  // refusal is disarmed from then on
  bool refuse_now() {
    if (refuse_in_.load(std::memory_order_relaxed) <= 0) return false;   // the usual case: one relaxed load
    std::lock_guard<std::mutex> lock(mu_);
    const int64_t left = refuse_in_.load(std::memory_order_relaxed);
    if (left <= 0) return false;
    refuse_in_.store(left - 1, std::memory_order_relaxed);
    return left == 1;
  }

  Stats stats() {
    std::lock_guard<std::mutex> lock(mu_);
    return Stats{(int64_t)live_.size(), live_bytes_, allocs_, frees_, streams_.load(std::memory_order_relaxed),
                 events_.load(std::memory_order_relaxed)};
  }

 private:
  std::mutex mu_;
  std::unordered_map<const void *, size_t> live_;
  int64_t live_bytes_ = 0, allocs_ = 0, frees_ = 0;
  std::atomic<int64_t> streams_{0}, events_{0};
  std::atomic<int64_t> refuse_in_{0};
};

DevLedger &dev_ledger();   // the library's one ledger (gpemu_api.hip)

}  // namespace gpemu
