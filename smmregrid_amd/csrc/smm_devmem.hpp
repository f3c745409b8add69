// Owners of the library's HBM and page-locked blocks, and the one place the ownership rule is written: a buffer holds
// at most one block, frees it when it is reset, assigned over or destroyed, and is EMPTY after a step of its own that
// failed (the block is freed there, the sticky HIP error cleared).  So a caller uploads into locals and moves them into
// a handle once every upload has succeeded: a failure on the way leaves the handle as it was and nothing to unwind.
// Host only.  No object of these types has static storage duration: nothing calls into HIP during process teardown.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace smm {

// n elements of T from hipMalloc
template <typename T>
class DeviceBuf {
 public:
  DeviceBuf() = default;
  DeviceBuf(DeviceBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DeviceBuf& operator=(DeviceBuf&& o) noexcept {   // frees what the target held
    DeviceBuf taken(std::move(o));
    std::swap(p_, taken.p_);
    std::swap(n_, taken.n_);
    return *this;
  }
  ~DeviceBuf() { reset(); }
  T* get() const { return p_; }
  size_t bytes() const { return n_ * sizeof(T); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  // frees what the buffer held, then allocates n elements
  hipError_t alloc(size_t n) {
    reset();
    const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
    if (e != hipSuccess) {
      p_ = nullptr;
      (void)hipGetLastError();
    } else {
      n_ = n;
    }
    return e;
  }
  // a device copy of h: at least one element is allocated, nothing is copied for an empty vector
  hipError_t upload(const std::vector<T>& h) {
    hipError_t e = alloc(h.empty() ? 1 : h.size());
    if (e == hipSuccess && !h.empty()) {
      e = hipMemcpy(p_, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        reset();
        (void)hipGetLastError();
      }
    }
    return e;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// bytes of page-locked host memory from hipHostMalloc(..., hipHostMallocDefault)
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {   // frees what the target held
    PinnedBuf taken(std::move(o));
    std::swap(p_, taken.p_);
    std::swap(n_, taken.n_);
    return *this;
  }
  ~PinnedBuf() { reset(); }
  void* get() const { return p_; }
  size_t bytes() const { return n_; }
  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  hipError_t alloc(size_t bytes) {
    reset();
    const hipError_t e = hipHostMalloc(&p_, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
      p_ = nullptr;
      (void)hipGetLastError();
    } else {
      n_ = bytes;
    }
    return e;
  }

 private:
  void* p_ = nullptr;
  size_t n_ = 0;
};

}  // namespace smm
