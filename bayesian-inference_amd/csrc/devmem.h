// Host-side ownership of device memory (included at the end of internal.h).  Every hipMalloc and hipFree of the library
// is in this header, and every one of them feeds the ledger (devledger.h), which also decides the tests' one-shot
// refusal before the allocator is called.  Three owners:
//   - a temporary that does not outlive the call: DevScope;
//   - a buffer a handle keeps and regrows on demand: dev_reserve;
//   - a fixed field of a handle: dev_alloc into the struct, dev_free in the handle's *_destroy.
// The rule of all three is "synchronise, then free": asynchronous copies into the caller's arrays and kernels in flight
// may still use a buffer when it goes -- an early return that unwinds a wrapper, a regrow between two launches.
#pragma once
#include <initializer_list>

#include "devledger.h"

namespace gpemu {

// the ledger's one-shot refusal, asked before any HIP call of an allocation
static inline int dev_alloc_refused(size_t bytes) {
  if (!dev_ledger().refuse_now()) return GPEMU_OK;
  set_error("device allocation of %zu bytes refused (gpemu_devmem_refuse_nth)", bytes);
  return GPEMU_ERR_HIP;
}

// every allocation of the library: one error text (the bytes asked for, HIP's reason)
static inline int dev_alloc_bytes(void **p, size_t bytes) {
  *p = nullptr;
  GP_TRY(dev_alloc_refused(bytes));
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    *p = nullptr;
    set_error("device allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    return GPEMU_ERR_HIP;
  }
  dev_ledger().note(*p, bytes);
  return GPEMU_OK;
}

// n elements of T; a request of 0 or fewer allocates one element, so that the pointer is always valid
template <typename T>
static size_t dev_bytes(int64_t n) { return sizeof(T) * (size_t)(n > 0 ? n : 1); }
template <typename T>
static int dev_alloc(T **p, int64_t n) { return dev_alloc_bytes((void **)p, dev_bytes<T>(n)); }

// n elements of uncached device memory (its values are written by other workgroups or other GPUs and polled), or, where
// the runtime has none to give, of plain device memory: *uncached tells which
template <typename T>
static int dev_alloc_uncached(T **p, int64_t n, bool *uncached) {
  *p = nullptr;
  *uncached = false;
  GP_TRY(dev_alloc_refused(dev_bytes<T>(n)));   // one allocation, whichever branch serves it
  *uncached = hipExtMallocWithFlags((void **)p, dev_bytes<T>(n), hipDeviceMallocUncached) == hipSuccess;
  if (*uncached) {
    dev_ledger().note((void *)*p, dev_bytes<T>(n));
    return GPEMU_OK;
  }
  (void)hipGetLastError();
  *p = nullptr;
  const hipError_t e = hipMalloc((void **)p, dev_bytes<T>(n));
  if (e != hipSuccess) {
    *p = nullptr;
    set_error("device allocation of %zu bytes failed: %s", dev_bytes<T>(n), hipGetErrorString(e));
    return GPEMU_ERR_HIP;
  }
  dev_ledger().note((void *)*p, dev_bytes<T>(n));
  return GPEMU_OK;
}

// frees a handle's field and nulls it.  The caller has synchronised whatever may still use it.
template <typename T>
static void dev_free(T *&p) {
  if (p) {
    dev_ledger().forget((const void *)p);
    (void)hipFree((void *)p);
  }
  p = nullptr;
}

// the streams and events a handle owns: created and destroyed here, so that the ledger counts them
static inline hipError_t stream_create(hipStream_t *st, unsigned flags) {
  const hipError_t e = hipStreamCreateWithFlags(st, flags);
  if (e == hipSuccess) dev_ledger().stream_made();
  return e;
}
static inline hipError_t stream_create(hipStream_t *st, unsigned flags, int priority) {
  const hipError_t e = hipStreamCreateWithPriority(st, flags, priority);
  if (e == hipSuccess) dev_ledger().stream_made();
  return e;
}
static inline hipError_t stream_create_cu_mask(hipStream_t *st, uint32_t words, const uint32_t *mask) {
  const hipError_t e = hipExtStreamCreateWithCUMask(st, words, mask);
  if (e == hipSuccess) dev_ledger().stream_made();
  return e;
}
static inline void stream_destroy(hipStream_t &st) {
  if (st) {
    (void)hipStreamDestroy(st);
    dev_ledger().stream_gone();
  }
  st = nullptr;
}
static inline hipError_t event_create(hipEvent_t *ev, unsigned flags = hipEventDefault) {
  const hipError_t e = hipEventCreateWithFlags(ev, flags);
  if (e == hipSuccess) dev_ledger().event_made();
  return e;
}
static inline void event_destroy(hipEvent_t &ev) {
  if (ev) {
    (void)hipEventDestroy(ev);
    dev_ledger().event_gone();
  }
  ev = nullptr;
}

// asynchronous copy of n elements from host memory, which the caller keeps alive until `st` is synchronised
template <typename T>
static int upload(T *dst, const T *src, int64_t n, hipStream_t st) {
  GP_HIP(hipMemcpyAsync(dst, src, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, st));
  return GPEMU_OK;
}

// Owner of the device buffers of one call, which works on the stream `st`.  The destructor synchronises `st` and then
// frees what the scope still holds, in the order of allocation, ignoring errors: whichever way the call returns,
// nothing is freed under a copy or a kernel.
class DevScope {
 public:
  explicit DevScope(hipStream_t st) : st_(st) {}
  DevScope(const DevScope &) = delete;
  DevScope &operator=(const DevScope &) = delete;
  ~DevScope() {
    if (held_.empty()) return;
    (void)hipStreamSynchronize(st_);
    for (void *q : held_) {
      dev_ledger().forget(q);
      (void)hipFree(q);
    }
  }
  template <typename T>
  int alloc(T **p, int64_t n) {
    GP_TRY(dev_alloc(p, n));
    held_.push_back((void *)*p);
    return GPEMU_OK;
  }
  template <typename T>
  int alloc_uncached(T **p, int64_t n, bool *uncached) {
    GP_TRY(dev_alloc_uncached(p, n, uncached));
    held_.push_back((void *)*p);
    return GPEMU_OK;
  }
  // gives p up to a longer-lived owner (the block stays live in the ledger)
  template <typename T>
  T *release(T *p) {
    for (size_t i = 0; i < held_.size(); ++i)
      if (held_[i] == (void *)p) { held_.erase(held_.begin() + (std::ptrdiff_t)i); break; }
    return p;
  }
  // asynchronous copy of n elements to host memory, on the scope's stream
  template <typename T>
  int download(T *host, const T *dev, int64_t n) {
    GP_HIP(hipMemcpyAsync(host, dev, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, st_));
    return GPEMU_OK;
  }

 private:
  hipStream_t st_;
  std::vector<void *> held_;
};

// "These fields of a handle must hold `need` (in the unit of *cap)."  A capacity that suffices returns before any HIP
// call.  Otherwise: synchronise `streams` (every stream whose work may still read the old buffers), free and null the
// fields, allocate them anew, and store the capacity once all of them exist.
struct DevField { void **p; size_t bytes; };
template <typename T>
static DevField dev_field(T **p, int64_t n) { return DevField{(void **)p, dev_bytes<T>(n)}; }
template <typename T>
static DevField dev_field_bytes(T **p, size_t bytes) { return DevField{(void **)p, bytes ? bytes : 8}; }

template <typename C>
static int dev_reserve(C *cap, C need, std::initializer_list<hipStream_t> streams, const DevField *fields, size_t nfields) {
  if (need <= *cap) return GPEMU_OK;
  for (hipStream_t st : streams) GP_HIP(hipStreamSynchronize(st));
  for (size_t i = 0; i < nfields; ++i) dev_free(*fields[i].p);
  *cap = 0;
  for (size_t i = 0; i < nfields; ++i) GP_TRY(dev_alloc_bytes(fields[i].p, fields[i].bytes));
  *cap = need;
  return GPEMU_OK;
}
template <typename C>
static int dev_reserve(C *cap, C need, std::initializer_list<hipStream_t> streams, std::initializer_list<DevField> fields) {
  return dev_reserve(cap, need, streams, fields.begin(), fields.size());
}

}  // namespace gpemu
