// Host-side helpers every ring export repeats: the device of the calling thread for the length
// of a call, and the ring-depth check.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rocmdash {

struct DeviceScope {  // the calling thread's device, restored on exit
  int prev = -1, dev;
  explicit DeviceScope(int d) : dev(d) {
    (void)hipGetDevice(&prev);
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceScope() {
    if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
  }
};

inline bool pow2(uint64_t x) { return x != 0 && (x & (x - 1)) == 0; }

}  // namespace rocmdash
