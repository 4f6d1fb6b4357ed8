// Host-side HIP plumbing of rt_api.hip and ppm_api.hip: error checking, the device guard, the
// exception -> return code mapping, and move-only owners of device arrays, events and streams.
// Everything has internal linkage: both libraries can be loaded into one process and share none
// of it (each keeps its own thread_local error string and passes its set_error to guarded_with).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <ios>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ceng795_rt.h"  // RT_E_*

namespace {

struct HipFailure {
  hipError_t err;
  const char* what;
};

void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw HipFailure{e, what};
}

// Makes `dev` current for a scope.  A failed hipGetDevice leaves prev = -1 and nothing is
// restored.  The std::nothrow form ignores a failed hipSetDevice too (destructors).
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) hip_check(hipSetDevice(dev), "hipSetDevice");
  }
  DeviceGuard(int dev, const std::nothrow_t&) noexcept {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
  ~DeviceGuard() {
    int cur;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// Runs f and maps what it throws to an RT_E_* code through the library's own set_error.
template <typename SetError, typename F>
int guarded_with(SetError&& set_error, F&& f) {
  try {
    return f();
  } catch (const HipFailure& h) {
    return set_error(RT_E_HIP, std::string(h.what) + ": " + hipGetErrorString(h.err));
  } catch (const std::domain_error& e) {
    return set_error(RT_E_UNSUPPORTED, e.what());
  } catch (const std::invalid_argument& e) {
    return set_error(RT_E_INVALID, e.what());
  } catch (const std::ios_base::failure& e) {
    return set_error(RT_E_IO, e.what());
  } catch (const std::runtime_error& e) {
    return set_error(RT_E_PARSE, e.what());
  } catch (const std::bad_alloc&) {
    return set_error(RT_E_INVALID, "out of host memory");
  } catch (const std::exception& e) {
    return set_error(RT_E_INVALID, e.what());
  }
}

// Grow-only device array of `cap` elements; frees it when it goes.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  // a buffer of another element type, taken over as whole Ts (a list of uploads: DevBuf<char>)
  template <typename U>
  explicit DevBuf(DevBuf<U>&& o) noexcept
      : p(reinterpret_cast<T*>(o.p)), cap(o.cap * sizeof(U) / sizeof(T)) {
    o.p = nullptr, o.cap = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void reserve(size_t n, const char* what) {
    if (n <= cap) return;
    release();
    hip_check(hipMalloc(&p, n * sizeof(T)), what);
    cap = n;
  }
  void release() {
    (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// v on the current device, in an allocation of max(its bytes + pad_bytes, 16) bytes.
template <typename T>
DevBuf<T> upload(const std::vector<T>& v, const char* what, size_t pad_bytes) {
  DevBuf<T> b;
  hip_check(hipMalloc(&b.p, std::max<size_t>(v.size() * sizeof(T) + pad_bytes, 16)), what);
  b.cap = v.size();
  if (!v.empty()) hip_check(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), what);
  return b;
}

// An event, made by create() (once; flags as hipEventCreateWithFlags) and destroyed with its owner.
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  void create(unsigned flags = hipEventDefault, const char* what = "event") {
    if (!e) hip_check(hipEventCreateWithFlags(&e, flags), what);
  }
  operator hipEvent_t() const { return e; }
};

// A non-blocking stream, made by create() (once) and destroyed with its owner.
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  void create(const char* what = "stream") {
    if (!s) hip_check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), what);
  }
  operator hipStream_t() const { return s; }
};

}  // namespace
