// device_buffer.hpp -- a device allocation together with its element count (host side only).
// Every hipMalloc / hipFree of the runtime goes through this type: the size a buffer was allocated with is the size it is
// cloned and freed with.  No implicit conversion to T*: "allocated" and "null" stay visible at every use (buf.p).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace rtoc {

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;        // elements allocated (or bound)
  bool owned = false;  // freed by release(); false for a caller's memory (bind)

  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr), n = std::exchange(o.n, 0), owned = std::exchange(o.owned, false);
    }
    return *this;
  }
  ~DevBuf() { release(); }

  // hipFree / hipMalloc synchronise the device: callers keep both away from forked streams and captured regions
  void release() {
    if (owned && p) (void)hipFree(p);
    p = nullptr, n = 0, owned = false;
  }
  // exactly `count` elements: nothing to do if that is what is there, else a new allocation (contents are not kept)
  hipError_t reserve(size_t count, bool* fresh = nullptr) {
    if (fresh) *fresh = false;
    if (p && n == count) return hipSuccess;
    release();
    const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    n = count, owned = true;
    if (fresh) *fresh = true;
    return hipSuccess;
  }
  // at least `count` elements: scratch that only ever grows
  hipError_t grow(size_t count) { return (p && n >= count) ? hipSuccess : reserve(count); }
  // the capacity and the contents of src (nothing if src was never allocated)
  hipError_t copy_from(const DevBuf& src, hipStream_t s) {
    if (!src.p) return hipSuccess;
    const hipError_t e = reserve(src.n);
    return e != hipSuccess ? e : hipMemcpyAsync(p, src.p, n * sizeof(T), hipMemcpyDeviceToDevice, s);
  }
  void bind(T* external, size_t count) {
    release();
    p = external, n = count, owned = false;
  }
};

}  // namespace rtoc
