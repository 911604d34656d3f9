// khr_owned.h — move-only owners of the HIP resources a context holds (host code only).
// The rule of this library: a member either IS one of these owners, or it is a view into memory somebody else owns and says
// so.  hipMalloc / hipFree, hipHostMalloc / hipHostFree, hipEventCreate* / hipEventDestroy and hipStreamCreate* /
// hipStreamDestroy are called here and nowhere else.  The owners return the KHR_* codes and leave the error text behind like
// every other call of the C ABI; they convert to the raw pointer / handle, so use sites read as with raw members.
// Every owner counts what it holds in g_live (khr_debug_live_resources): the leak tests read the four counts.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/khronos_amd.h"

extern "C" void khr_set_last_error(const char* text);  // khronos_amd.hip

namespace khr {

enum LiveKind { LIVE_DEVICE = 0, LIVE_PINNED = 1, LIVE_EVENT = 2, LIVE_STREAM = 3 };
inline std::atomic<int64_t> g_live[4];
inline void liveAdd(LiveKind k, int64_t d) { g_live[k].fetch_add(d, std::memory_order_relaxed); }

inline int ownedFail(int code, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  khr_set_last_error(buf);
  return code;
}

template <typename T> constexpr size_t kOwnedEltBytes = sizeof(T);
template <> inline constexpr size_t kOwnedEltBytes<void> = 1;  // (untyped staging blocks count bytes)

// `count` elements of device memory (PINNED = false) or of page-locked host memory with its device view (PINNED = true)
template <typename T, bool PINNED>
class OwnedBuf {
 public:
  OwnedBuf() = default;
  OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_), dev_(o.dev_), n_(o.n_) { o.p_ = o.dev_ = nullptr, o.n_ = 0; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, dev_ = o.dev_, n_ = o.n_;
      o.p_ = o.dev_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  ~OwnedBuf() { reset(); }

  // exactly `count` elements, uninitialised; whatever was held is released first, and a failure leaves the object empty
  int alloc(size_t count) {
    reset();
    if (count == 0) return KHR_OK;  // (nothing to hold: empty, as the runtime's own zero-size allocation is)
    const size_t bytes = count * kOwnedEltBytes<T>;
    void* p = nullptr;
    const hipError_t e = PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e != hipSuccess || !p) return ownedFail(KHR_ENOMEM, "%s(%zu bytes) failed: %s", PINNED ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
    liveAdd(PINNED ? LIVE_PINNED : LIVE_DEVICE, 1);
    p_ = static_cast<T*>(p), n_ = count;
    if (PINNED) {
      void* d = nullptr;
      const hipError_t eg = hipHostGetDevicePointer(&d, p, 0);
      if (eg != hipSuccess) {
        reset();
        return ownedFail(KHR_EDEVICE, "hipHostGetDevicePointer failed: %s", hipGetErrorString(eg));
      }
      dev_ = static_cast<T*>(d);
    }
    return KHR_OK;
  }
  // grow-only: nothing happens while `count` fits.  The caller waits first for whatever still uses the old block.
  int reserve(size_t count) { return count <= n_ ? KHR_OK : alloc(count); }
  void reset() {
    if (p_) {
      if (PINNED) (void)hipHostFree(p_); else (void)hipFree(p_);
      liveAdd(PINNED ? LIVE_PINNED : LIVE_DEVICE, -1);
    }
    p_ = dev_ = nullptr, n_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* dev() const {  // the kernels' view of a page-locked block (fetched once, at allocation)
    static_assert(PINNED, "dev() is the device view of page-locked memory");
    return dev_;
  }
  size_t count() const { return n_; }

 private:
  T* p_ = nullptr;
  T* dev_ = nullptr;
  size_t n_ = 0;
};
template <typename T> using DevBuf = OwnedBuf<T, false>;
template <typename T> using PinnedBuf = OwnedBuf<T, true>;

// a runtime handle that is destroyed with `Destroy` when owned; a handle that is only referred to is left alone and not counted
template <typename H, hipError_t (*Destroy)(H), LiveKind KIND>
class OwnedHandle {
 public:
  OwnedHandle() = default;
  OwnedHandle(OwnedHandle&& o) noexcept : h_(o.h_), own_(o.own_) { o.h_ = nullptr, o.own_ = false; }
  OwnedHandle& operator=(OwnedHandle&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_, own_ = o.own_;
      o.h_ = nullptr, o.own_ = false;
    }
    return *this;
  }
  OwnedHandle(const OwnedHandle&) = delete;
  OwnedHandle& operator=(const OwnedHandle&) = delete;
  ~OwnedHandle() { reset(); }
  void reset() {
    if (h_ && own_) {
      (void)Destroy(h_);
      liveAdd(KIND, -1);
    }
    h_ = nullptr, own_ = false;
  }
  H get() const { return h_; }
  operator H() const { return h_; }

 protected:
  int adopt(hipError_t e, const char* what) {  // the outcome of a create call that wrote h_
    if (e != hipSuccess) {
      h_ = nullptr;
      return ownedFail(KHR_EDEVICE, "%s failed: %s", what, hipGetErrorString(e));
    }
    own_ = true;
    liveAdd(KIND, 1);
    return KHR_OK;
  }
  H h_ = nullptr;
  bool own_ = false;
};

class Event : public OwnedHandle<hipEvent_t, hipEventDestroy, LIVE_EVENT> {
 public:
  // created at the first call (without timing unless the caller measures with it); later calls do nothing
  int ensure(unsigned flags = hipEventDisableTiming) { return h_ ? KHR_OK : adopt(hipEventCreateWithFlags(&h_, flags), "hipEventCreate"); }
};

class Stream : public OwnedHandle<hipStream_t, hipStreamDestroy, LIVE_STREAM> {
 public:
  // a stream of its own; `priority` = nullptr: the default priority
  int create(unsigned flags, const int* priority = nullptr) {
    reset();
    return adopt(priority ? hipStreamCreateWithPriority(&h_, flags, *priority) : hipStreamCreateWithFlags(&h_, flags), "hipStreamCreate");
  }
  // a caller's stream: used, never destroyed, not counted
  void refer(hipStream_t s) {
    reset();
    h_ = s;
  }
  bool owns() const { return own_; }
};

}  // namespace khr
