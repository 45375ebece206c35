// Owning side buffers of the engine: one move-only type for device memory and pinned host memory. A buffer owns its
// allocation and nothing else -- WHEN it may be replaced (the stream idle, the graphs that hold its address dropped) is
// the caller's business (engine.h: Engine::side_alloc). The destructor frees; the engine still releases in its own order
// (Engine::free_all), the destructors are the net under error paths.
#pragma once
#include <cstring>
#include <string>

#include "pe_rt.h"

namespace pe {

struct DeviceMem {
  static constexpr const char* name = "hipMalloc";
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { hipFree(p); }
  static hipError_t zero(void* p, size_t bytes) { return hipMemset(p, 0, bytes); }
};
struct PinnedMem {
  static constexpr const char* name = "hipHostMalloc";
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
  static void release(void* p) { hipHostFree(p); }
  static hipError_t zero(void* p, size_t bytes) { memset(p, 0, bytes); return hipSuccess; }
};

template <typename T, class Mem>
class Buffer {
 public:
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  Buffer(Buffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~Buffer() { reset(); }

  T* get() const { return p_; }
  size_t size() const { return n_; }                   // capacity in elements
  size_t bytes() const { return n_ * sizeof(T); }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() {
    if (p_) Mem::release(p_);
    p_ = nullptr; n_ = 0;
  }
  // At least n elements, the content not kept; returns whether it allocated (an allocation of exactly n). `what`: a failure
  // throws "out of device memory: N MiB of <what>", N from what_bytes where one error speaks for several buffers; null: the
  // HIP error is thrown as it is. A failed allocation leaves the buffer empty.
  bool grow(size_t n, const char* what = nullptr, size_t what_bytes = 0) {
    if (p_ && n <= n_) return false;
    reset();
    void* p = nullptr;
    const hipError_t e = Mem::alloc(&p, n * sizeof(T));
    if (e != hipSuccess && what) {
      (void)hipGetLastError();
      throw std::runtime_error("out of device memory: " + std::to_string((what_bytes ? what_bytes : n * sizeof(T)) >> 20) + " MiB of " + what);
    }
    if (e != hipSuccess) throw std::runtime_error(std::string(Mem::name) + ": " + hipGetErrorString(e));
    p_ = static_cast<T*>(p); n_ = n;
    return true;
  }
  void zero() { PE_HIP(Mem::zero(p_, bytes())); }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

template <typename T> using DevBuf = Buffer<T, DeviceMem>;
template <typename T> using PinBuf = Buffer<T, PinnedMem>;

}  // namespace pe
