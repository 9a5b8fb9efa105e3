// Owners of what a LongWindowSet allocates: device buffers, mapped pinned host buffers,
// events, the capture stream and the graph. Move-only; each releases what it holds, so a
// throw halfway through an allocation sequence frees what came before it and the set's
// destructor lists nothing by hand.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>

namespace rocmdash {

inline void lw_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// hipMalloc / hipFree. fill: the byte every byte starts as (0, or 0xFF: NaN floats); -1
// leaves the memory as it came.
class LwDeviceBuf {
 public:
  LwDeviceBuf() = default;
  explicit LwDeviceBuf(size_t bytes, int fill = -1, const char* what = "hipMalloc") : bytes_(bytes) {
    lw_check(hipMalloc(&p_, bytes), what);
    if (fill >= 0) this->fill(fill);
  }
  LwDeviceBuf(LwDeviceBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  LwDeviceBuf& operator=(LwDeviceBuf&& o) noexcept {
    if (this != &o) {
      release();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  ~LwDeviceBuf() { release(); }
  explicit operator bool() const { return p_ != nullptr; }
  template <class T = void>
  T* get() const {
    return static_cast<T*>(p_);
  }
  size_t bytes() const { return bytes_; }
  void fill(int byte) {  // synchronous (hipMemset), the whole buffer
    const hipError_t e = hipMemset(p_, byte, bytes_);
    if (e != hipSuccess) {  // also reached from the constructor, whose throw runs no destructor
      release();
      lw_check(e, "hipMemset");
    }
  }

 private:
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

// hipHostMalloc (flags: hipHostMallocMapped, with or without Coherent) / hipHostFree, and
// the buffer as the device sees it. need_dev: no device view is an error (else dev() is
// null and the caller takes another path).
class LwHostBuf {
 public:
  LwHostBuf() = default;
  LwHostBuf(size_t bytes, unsigned flags, bool zero, bool need_dev) {
    lw_check(hipHostMalloc(&h_, bytes, flags), "hipHostMalloc");
    if (zero) std::memset(h_, 0, bytes);
    const hipError_t e = hipHostGetDevicePointer(&d_, h_, 0);
    if (e != hipSuccess) {
      d_ = nullptr;
      if (need_dev) {
        release();
        lw_check(e, "hipHostGetDevicePointer");
      }
    }
  }
  LwHostBuf(LwHostBuf&& o) noexcept : h_(std::exchange(o.h_, nullptr)), d_(std::exchange(o.d_, nullptr)) {}
  LwHostBuf& operator=(LwHostBuf&& o) noexcept {
    if (this != &o) {
      release();
      h_ = std::exchange(o.h_, nullptr);
      d_ = std::exchange(o.d_, nullptr);
    }
    return *this;
  }
  ~LwHostBuf() { release(); }
  explicit operator bool() const { return h_ != nullptr; }
  template <class T = void>
  T* host() const {
    return static_cast<T*>(h_);
  }
  template <class T = void>
  T* dev() const {
    return static_cast<T*>(d_);
  }

 private:
  void release() {
    if (h_) (void)hipHostFree(h_);
    h_ = d_ = nullptr;
  }
  void* h_ = nullptr;
  void* d_ = nullptr;
};

// an event, a stream, a graph or its executable: destroyed with the owner
template <class H, hipError_t (*Destroy)(H)>
class LwHandle {
 public:
  LwHandle() = default;
  explicit LwHandle(H h) : h_(h) {}
  LwHandle(LwHandle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  LwHandle& operator=(LwHandle&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  ~LwHandle() { reset(); }
  explicit operator bool() const { return h_ != nullptr; }
  H get() const { return h_; }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }

 private:
  H h_ = nullptr;
};
using LwEvent = LwHandle<hipEvent_t, hipEventDestroy>;
using LwStream = LwHandle<hipStream_t, hipStreamDestroy>;
using LwGraph = LwHandle<hipGraph_t, hipGraphDestroy>;
using LwGraphExec = LwHandle<hipGraphExec_t, hipGraphExecDestroy>;

inline LwEvent lw_make_event(unsigned flags) {
  hipEvent_t e = nullptr;
  lw_check(hipEventCreateWithFlags(&e, flags), "hipEventCreate");
  return LwEvent(e);
}

}  // namespace rocmdash
