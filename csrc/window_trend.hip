// Per-column {min, max, mean, count} of the windows in the time-major device rings (see
// window_trend.h).
#include "window_trend.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_scope.h"
#include "device_window.h"
#include "long_window.h"
#include "long_window_dev.h"

namespace rocmdash {
namespace {

constexpr int kWaveNT = 256;    // small slots: one wave64 per (ring, slot), 4 slots per workgroup
constexpr int kGroupNT = 1024;  // large slots: one workgroup of 16 waves per (ring, slot)
constexpr int kUnroll = 8;      // loads a lane has in flight before it counts any of them
// a slot of at most this many floats is streamed by one wave (<= 4 rounds of kUnroll loads)
constexpr uint32_t kWaveSlotFloats = 64 * kUnroll * 4;

struct TrendRing {
  const float* base;  // device ring: row r at base + (r & mask) * stride
  float* dst;         // the ring's first series' [P + 1][4]
  uint64_t head;
  uint32_t stride, cols, mask, n;
};

struct TrendArgs {
  TrendRing r[kTrendRingsPerLaunch];  // blockIdx.y
  uint32_t log2c, P;
};

struct TrendAcc {
  double sum;
  uint32_t mn, mx, cnt;  // order-preserving keys
};

__device__ __forceinline__ void trend_merge(TrendAcc& a, const TrendAcc& b) {
  a.sum += b.sum;
  a.mn = min(a.mn, b.mn);
  a.mx = max(a.mx, b.mx);
  a.cnt += b.cnt;
}

// The rows of slot j (window_trend.h; rocmdash.ops.window_trend.trend_geometry states the
// same): [lo, hi), lo == hi when the slot is empty. Uniform.
__device__ __forceinline__ void trend_slot_rows(uint64_t head, uint32_t n, uint32_t log2c, uint32_t P, uint32_t j,
                                                uint64_t& lo, uint64_t& hi) {
  lo = hi = 0;
  if (n == 0 || head == 0) return;
  const int64_t a = int64_t((head - 1) >> log2c) - int64_t(P) + int64_t(j);
  if (a < 0) return;
  const uint64_t b = max(uint64_t(a) << log2c, head - n), e = min((uint64_t(a) + 1) << log2c, head);
  if (b < e) {
    lo = b;
    hi = e;
  }
}

// One slot of one ring by NW waves (this one is `wave`): the slot's block of rows x stride
// contiguous floats is cut into pieces of L floats - L the largest multiple of the stride a
// wave holds, so lane l stays on series l % stride - and wave w streams the pieces w, w + NW,
// ...: coalesced 4-byte loads (a row of 1 to 16 floats is not 16-byte aligned in general),
// kUnroll of them in flight per lane. Lanes of one series are then reduced in a fixed tree
// order, the waves in wave order through LDS: the same bits for the same data.
template <int NW>
__device__ __forceinline__ void trend_slot(const TrendRing& R, uint32_t log2c, uint32_t P, uint32_t j, uint32_t lane,
                                           uint32_t wave, TrendAcc (*sh)[kMaxTrendStride]) {
  uint64_t lo, hi;
  trend_slot_rows(R.head, R.n, log2c, P, j, lo, hi);
  const uint32_t stride = R.stride;
  const uint32_t F = uint32_t(hi - lo) * stride;  // <= 65536 x 64 floats
  const uint32_t per = 64u / stride;              // lanes per series
  const uint32_t L = per * stride;
  const float* p = R.base + size_t(lo & R.mask) * stride;

  TrendAcc acc{0.0, 0xFFFFFFFFu, 0u, 0u};
  if (lane < L) {
    for (uint32_t k0 = wave; uint64_t(k0) * L < F; k0 += NW * kUnroll) {
      float v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint64_t i = uint64_t(k0 + uint32_t(u) * NW) * L + lane;
        v[u] = i < F ? p[i] : __builtin_nanf("");
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const float x = v[u];
        if (isnan(x)) continue;  // invalid samples, pieces past the slot
        const uint32_t k = fkey(x);
        acc.sum += double(x);
        acc.mn = min(acc.mn, k);
        acc.mx = max(acc.mx, k);
        ++acc.cnt;
      }
    }
  }
  // the series' lanes l, l + stride, ...: a tree over their index, so lane l < stride ends
  // with the wave's partial of series l
  const uint32_t idx = lane / stride;
  for (uint32_t off = per > 1 ? 1u << (31 - __builtin_clz(per - 1)) : 0u; off >= 1; off >>= 1) {
    const int src = int(lane + off * stride) & 63;
    TrendAcc o;
    o.sum = __shfl(acc.sum, src);
    o.mn = uint32_t(__shfl(int(acc.mn), src));
    o.mx = uint32_t(__shfl(int(acc.mx), src));
    o.cnt = uint32_t(__shfl(int(acc.cnt), src));
    if (lane < L && idx + off < per) trend_merge(acc, o);
  }
  if constexpr (NW > 1) {
    if (lane < R.cols) sh[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    if (lane < R.cols) {
      acc = sh[0][lane];
      for (int w = 1; w < NW; ++w) trend_merge(acc, sh[w][lane]);
    }
  }
  if (lane < R.cols) {
    const float nan = __builtin_nanf("");
    float4 o{nan, nan, nan, 0.f};
    if (acc.cnt) o = float4{kfloat(acc.mn), kfloat(acc.mx), float(acc.sum / double(acc.cnt)), float(acc.cnt)};
    reinterpret_cast<float4*>(R.dst)[size_t(lane) * (P + 1) + j] = o;
  }
}

// grid (slots, rings): blockIdx.y picks the ring from the by-value argument (uniform: scalar loads)
__global__ __launch_bounds__(kWaveNT) void trend_wave_kernel(const TrendArgs a) {
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
  const uint32_t j = blockIdx.x * (kWaveNT / 64) + wave;
  if (j > a.P) return;  // whole waves; this kernel has no barrier
  trend_slot<1>(a.r[blockIdx.y], a.log2c, a.P, j, threadIdx.x & 63u, 0u, nullptr);
}

__global__ __launch_bounds__(kGroupNT) void trend_group_kernel(const TrendArgs a) {
  __shared__ TrendAcc sh[kGroupNT / 64][kMaxTrendStride];
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
  trend_slot<kGroupNT / 64>(a.r[blockIdx.y], a.log2c, a.P, blockIdx.x, threadIdx.x & 63u, wave, sh);
}

inline uint32_t log2u(uint32_t x) { return 31u - uint32_t(__builtin_clz(x)); }
inline bool bad_columns(uint32_t P) { return P < kMinTrendColumns || P > kMaxTrendColumns || !pow2(P); }
inline bool bad_dst(const float* dst) { return dst == nullptr || (reinterpret_cast<uintptr_t>(dst) & 15u) != 0; }

// rings [0, n) of `a` (every field set, all with rows_per_col = 1 << a.log2c)
void launch(const TrendArgs& a, uint32_t n, hipStream_t stream) {
  uint32_t floats = 0;
  for (uint32_t i = 0; i < n; ++i) floats = std::max(floats, a.r[i].stride << a.log2c);
  if (floats <= kWaveSlotFloats)
    hipLaunchKernelGGL(trend_wave_kernel, dim3((a.P + 1 + kWaveNT / 64 - 1) / (kWaveNT / 64), n), dim3(kWaveNT), 0, stream,
                       a);
  else
    hipLaunchKernelGGL(trend_group_kernel, dim3(a.P + 1, n), dim3(kGroupNT), 0, stream, a);
}

// One export over a set's rings: ring(i, &R) fills base / stride / cols / mask / head / n and
// returns the ring's first series.
template <class Ring>
int export_rings(size_t nrings, uint32_t window, uint32_t P, float* dst, hipStream_t stream, Ring ring) {
  TrendArgs a{};
  a.P = P;
  a.log2c = log2u(window / P);
  uint32_t n = 0;
  for (size_t i = 0; i < nrings; ++i) {
    TrendRing& R = a.r[n];
    const uint32_t first = ring(i, R);
    R.dst = dst + size_t(first) * (P + 1) * 4;
    if (++n == uint32_t(kTrendRingsPerLaunch) || i + 1 == nrings) {
      launch(a, n, stream);
      n = 0;
    }
  }
  return hipGetLastError();
}

}  // namespace

int launch_trend_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                      uint32_t P, uint32_t rows_per_col, float* dst, void* stream_ptr) {
  if (bad_columns(P) || bad_dst(dst) || base == nullptr || !pow2(depth) || rows_per_col < 1 ||
      rows_per_col > kMaxTrendRowsPerColumn || depth % rows_per_col != 0 || n > depth || n > head ||
      uint64_t(n) > uint64_t(P) * rows_per_col || stride < 1 || stride > kMaxTrendStride || cols < 1 || cols > stride)
    return hipErrorInvalidValue;
  TrendArgs a{};
  a.P = P;
  a.log2c = log2u(rows_per_col);  // a divisor of a power of two
  a.r[0] = TrendRing{base, dst, head, stride, cols, depth - 1, n};
  launch(a, 1, static_cast<hipStream_t>(stream_ptr));
  return hipGetLastError();
}

// DeviceWindowSet::export_trend lives here with its kernel (device_window.h declares it)
int DeviceWindowSet::export_trend(uint32_t P, float* dst, void* stream_ptr) const {
  if (bad_columns(P) || P > window_ || window_ / P > kMaxTrendRowsPerColumn || bad_dst(dst)) return hipErrorInvalidValue;
  for (const auto& r : rings_)
    if (r.ring->width() > kMaxTrendStride) return hipErrorInvalidValue;
  DeviceScope scope(device_);
  return export_rings(rings_.size(), window_, P, dst, static_cast<hipStream_t>(stream_ptr), [&](size_t i, TrendRing& R) {
    const auto& r = rings_[i];
    // the host mirrors of the last refresh: its kernel left rows [last_head - last_n,
    // last_head) in the device ring (entering rows it pulled or got by value included)
    R.base = r.dev;
    R.stride = R.cols = r.ring->width();
    R.mask = uint32_t(dev_rows() - 1);
    R.head = r.state_valid ? r.last_head : 0;
    R.n = r.state_valid ? r.last_n : 0;
    return r.first_series;
  });
}

// LongWindowSet::export_trend: the window the last refresh() left on the device is rows
// [copied - min(copied, W), copied) - stage() copies (or NaN-fills, for rows the host ring
// lost) everything up to the head it read and its refresh uses n = min(head, W) of it.
int LongWindowSet::export_trend(uint32_t P, float* dst, void* stream_ptr) {
  if (bad_columns(P) || P > window_ || window_ / P > kMaxTrendRowsPerColumn || bad_dst(dst)) return hipErrorInvalidValue;
  if (ingest_pending_) return hipErrorNotReady;  // staged rows no kernel has written yet: refresh() first
  DeviceScope scope(device_);
  return export_rings(rings_.size(), window_, P, dst, static_cast<hipStream_t>(stream_ptr), [&](size_t i, TrendRing& R) {
    const auto& r = rings_[i];
    R.base = r.dev.get<float>();
    R.stride = R.cols = r.ring->width();
    R.mask = window_ - 1;
    R.head = r.copied;
    R.n = uint32_t(std::min<uint64_t>(r.copied, window_));
    return r.first_series;
  });
}

}  // namespace rocmdash
