// device_mem.h — who owns device memory on the host side.  Two types, and the only hipMalloc / hipFree of the library:
//
//   DevBuf<T>   one grow-only allocation held by a long-lived object (a context, a scorer, a search).  Its one unit of
//               capacity is its own: size() in elements, bytes() in bytes.
//   DevArena    the temporaries of one call: get<T>(count) allocates, and whatever it handed out is freed on every way
//               out of the scope, early returns and exceptions included.
//
// and, beside them, the owner of the timing events of a call or of a scratch:
//
//   DevEvents<N>  N events, created on demand by create() and destroyed with their owner.
//
// Neither memory type pools, caches, copies or grows geometrically: an allocation is exactly what was asked for.  A failure is
// reported by value (false / nullptr); dev_alloc_failed() words it, and every caller returns it as HH_ERR_NOMEM.
// Needs the HIP runtime API and the standard library only, so a host compiler can build it alone.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

namespace {

inline std::string dev_alloc_failed(size_t bytes) { return "device allocation of " + std::to_string(bytes) + " bytes failed"; }

template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;             // a buffer passed by value (a launch's argument list) does not compile
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  // At least `count` elements.  A buffer that is large enough is left alone; otherwise the old one is freed FIRST (its
  // contents are not kept) and exactly `count` elements are allocated.  false: the buffer is empty, size() == 0.
  bool ensure(size_t count) {
    if (count <= n_ && p_) return true;
    reset();
    void* v = nullptr;
    if (hipMalloc(&v, count * sizeof(T)) != hipSuccess) return false;
    p_ = static_cast<T*>(v);
    n_ = count;
    return true;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }          // pointer arithmetic and kernel arguments read as they did on a raw pointer
  size_t size() const { return n_; }
  size_t bytes() const { return n_ * sizeof(T); }
  static size_t bytes_for(size_t count) { return count * sizeof(T); }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

class DevArena {
 public:
  DevArena() = default;
  DevArena(const DevArena&) = delete;
  DevArena& operator=(const DevArena&) = delete;
  ~DevArena() { release(); }

  // `count` elements, never fewer than one element nor than 16 bytes (a zero-sized request still gives a pointer a
  // kernel may be launched on).  nullptr: the allocation failed; the arena then hands out nullptr until release(), so a
  // run of get()s needs one ok() after it.
  template <class T>
  T* get(size_t count) {
    if (failed_) return nullptr;
    const size_t bytes = std::max<size_t>(std::max<size_t>(count, 1) * sizeof(T), 16);
    held_.reserve(held_.size() + 1);          // so that push_back cannot throw with an allocation in hand
    void* v = nullptr;
    if (hipMalloc(&v, bytes) != hipSuccess) {
      failed_ = bytes;
      return nullptr;
    }
    held_.push_back(v);
    return static_cast<T*>(v);
  }
  bool ok() const { return failed_ == 0; }
  size_t failed_bytes() const { return failed_; }   // of the request that failed
  void release() {                                  // frees now; the arena can be used again
    for (void* v : held_) (void)hipFree(v);
    held_.clear();
    failed_ = 0;
  }

 private:
  std::vector<void*> held_;
  size_t failed_ = 0;
};

template <int N>
class DevEvents {
 public:
  DevEvents() = default;
  DevEvents(const DevEvents&) = delete;
  DevEvents& operator=(const DevEvents&) = delete;
  ~DevEvents() {
    for (hipEvent_t e : ev_)
      if (e) (void)hipEventDestroy(e);
  }

  // Creates the events that do not exist yet (so a second call costs nothing); the first failure is returned and what was
  // created stays owned.
  hipError_t create() {
    for (hipEvent_t& e : ev_)
      if (!e) {
        const hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) {
          e = nullptr;
          return rc;
        }
      }
    return hipSuccess;
  }
  hipEvent_t operator[](int i) const { return ev_[i]; }

 private:
  hipEvent_t ev_[N] = {};
};

}  // namespace
