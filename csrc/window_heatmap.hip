// Per-column le-bucket bins of the windows in the time-major device rings (see
// window_heatmap.h).
#include "window_heatmap.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_scope.h"
#include "device_window.h"
#include "long_window.h"
#include "window_buckets.h"
#include "window_trend.h"

namespace rocmdash {
namespace {

constexpr int kWaveNT = 64;    // small slots: one wave64 = one workgroup per (ring, slot): the LDS below is one slot's
constexpr int kGroupNT = 512;  // large slots: one workgroup of 8 waves per (ring, slot); 4 of them share a CU: 32 waves
constexpr int kUnroll = 8;     // loads a lane has in flight before it bins any of them
// a slot of at most this many floats is streamed by one wave (<= 4 rounds of kUnroll loads)
constexpr uint32_t kWaveSlotFloats = 64 * kUnroll * 4;

struct HeatRing {
  const float* base;    // device ring: row r at base + (r & mask) * stride
  const float* bounds;  // the ring's first series' [B]
  int32_t* dst;         // ... [P + 1][B + 1]
  uint64_t head;
  uint32_t stride, cols, mask, n;
};

struct HeatArgs {
  HeatRing r[kHeatmapRingsPerLaunch];  // blockIdx.y
  uint32_t log2c, P, B;
};

// The rows of slot j, as trend_slot_rows of window_trend.hip (the one statement of them is
// rocmdash.ops.window_trend.trend_geometry): [lo, hi), lo == hi when the slot is empty. Uniform.
__device__ __forceinline__ void heat_slot_rows(uint64_t head, uint32_t n, uint32_t log2c, uint32_t P, uint32_t j,
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

// One slot of one ring by the NW waves of a workgroup. The stream is trend_slot's: the slot's
// block of rows x stride contiguous floats is cut into pieces of L floats - L the largest
// multiple of the stride a wave holds, so lane l stays on series l % stride - and wave w
// streams the pieces w, w + NW, ...: coalesced 4-byte loads, kUnroll of them in flight per
// lane. The binning is bucket_ring_kernel's: a lane keeps its current bin, the bin's edges
// (lo, hi] and the length of the run in registers; a sample that left the bin flushes the run
// to the lane's LDS counter [bin][lane] and finds its bin by a guess as if the bounds were
// evenly spaced, then a walk over the lane's own LDS column of the bounds - exact for any
// bounds. NaN edges stand for "no edge": bin 0 has no lower one, bin B no upper one. At the
// end the lanes of one series are summed and every (series, bin) of the slot is stored.
template <int NW>
__device__ __forceinline__ void heat_slot(const HeatRing& R, uint32_t log2c, uint32_t P, uint32_t B, uint32_t j,
                                          float* sb, uint32_t* cnt) {
  constexpr uint32_t NT = NW * 64;
  uint64_t rlo, rhi;
  heat_slot_rows(R.head, R.n, log2c, P, j, rlo, rhi);
  const uint32_t stride = R.stride;
  const uint32_t F = uint32_t(rhi - rlo) * stride;  // <= 65536 x 64 floats
  const uint32_t E = R.cols * (B + 1);              // the slot's counts
  if (F == 0) {                                     // uniform: the whole workgroup, before any barrier
    for (uint32_t e = threadIdx.x; e < E; e += NT) {
      const uint32_t c = e / (B + 1), k = e - c * (B + 1);
      R.dst[(size_t(c) * (P + 1) + j) * (B + 1) + k] = 0;
    }
    return;
  }
  const uint32_t per = 64u / stride;  // lanes per series
  const uint32_t L = per * stride;
  const float* p = R.base + size_t(rlo & R.mask) * stride;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = NW > 1 ? uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6))) : 0u;
  const float nan = __builtin_nanf("");

  for (uint32_t i = threadIdx.x; i < (B + 1) * 64u; i += NT) cnt[i] = 0u;
  for (uint32_t i = threadIdx.x; i < (B + 2) * 64u; i += NT) {
    const uint32_t k = i >> 6, l = i & 63u, c = l % stride;
    sb[i] = (k >= 1 && k <= B && l < L && c < R.cols) ? R.bounds[size_t(c) * B + (k - 1)] : nan;
  }
  __syncthreads();

  if (lane < L && lane % stride < R.cols) {  // columns >= cols are never read
    const float b0 = sb[64 + lane];
    const float inv = B > 1 ? float(B - 1) / (sb[B * 64 + lane] - b0) : 0.f;  // bins per unit
    uint32_t bin = 0, run = 0;
    float lo = nan, hi = b0;
    auto flush = [&] {
      if (!run) return;
      if constexpr (NW > 1)
        atomicAdd(&cnt[bin * 64 + lane], run);  // the column is shared by the waves
      else
        cnt[bin * 64 + lane] += run;
    };
    for (uint32_t k0 = wave; uint64_t(k0) * L < F; k0 += NW * kUnroll) {
      float v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint64_t i = uint64_t(k0 + uint32_t(u) * NW) * L + lane;
        v[u] = i < F ? p[i] : nan;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const float x = v[u];
        if (isnan(x)) continue;  // invalid samples, pieces past the slot
        if (x <= lo || hi < x) {
          flush();
          run = 0;
          // ceil((x - b0) x bins per unit) into [0, B]; inf and NaN (inf x 0) clamp too
          uint32_t g = uint32_t(fminf(fmaxf(ceilf((x - b0) * inv), 0.f), float(B)));
          lo = sb[g * 64 + lane];
          hi = sb[(g + 1) * 64 + lane];
          while (x <= lo) {  // ends at bin 0: its lo is NaN
            --g;
            hi = lo;
            lo = sb[g * 64 + lane];
          }
          while (hi < x) {  // ends at bin B: its hi is NaN
            ++g;
            lo = hi;
            hi = sb[(g + 1) * 64 + lane];
          }
          bin = g;
        }
        ++run;
      }
    }
    flush();
  }
  __syncthreads();

  // the slot's bin (c, k): the lanes c, c + stride, ...
  for (uint32_t e = threadIdx.x; e < E; e += NT) {
    const uint32_t c = e / (B + 1), k = e - c * (B + 1);
    uint32_t sum = 0;
    for (uint32_t i = 0; i < per; ++i) sum += cnt[k * 64 + c + i * stride];
    R.dst[(size_t(c) * (P + 1) + j) * (B + 1) + k] = int32_t(sum);
  }
}

// grid (slots, rings): blockIdx.y picks the ring from the by-value argument (uniform: scalar loads)
template <int NT>
__global__ __launch_bounds__(NT) void heatmap_kernel(const HeatArgs a) {
  __shared__ float sb[(kMaxBuckets + 2) * 64];      // [k][lane]: NaN, the lane's series' bounds, NaN
  __shared__ uint32_t cnt[(kMaxBuckets + 1) * 64];  // [bin][lane], shared by the waves
  heat_slot<NT / 64>(a.r[blockIdx.y], a.log2c, a.P, a.B, blockIdx.x, sb, cnt);
}

inline uint32_t log2u(uint32_t x) { return 31u - uint32_t(__builtin_clz(x)); }
inline bool bad_columns(uint32_t P) { return P < kMinTrendColumns || P > kMaxTrendColumns || !pow2(P); }
inline bool bad_buckets(const float* bounds, uint32_t B, const int32_t* dst) {
  return B < 1 || B > kMaxBuckets || bounds == nullptr || dst == nullptr || (reinterpret_cast<uintptr_t>(dst) & 3u) != 0;
}

// rings [0, n) of `a` (every field set, all with rows_per_col = 1 << a.log2c)
void launch(const HeatArgs& a, uint32_t n, hipStream_t stream) {
  uint32_t floats = 0;
  for (uint32_t i = 0; i < n; ++i) floats = std::max(floats, a.r[i].stride << a.log2c);
  if (floats <= kWaveSlotFloats)
    hipLaunchKernelGGL(heatmap_kernel<kWaveNT>, dim3(a.P + 1, n), dim3(kWaveNT), 0, stream, a);
  else
    hipLaunchKernelGGL(heatmap_kernel<kGroupNT>, dim3(a.P + 1, n), dim3(kGroupNT), 0, stream, a);
}

// One export over a set's rings: ring(i, &R) fills base / stride / cols / mask / head / n and
// returns the ring's first series.
template <class Ring>
int export_rings(size_t nrings, uint32_t window, uint32_t P, const float* bounds, uint32_t B, int32_t* dst,
                 hipStream_t stream, Ring ring) {
  HeatArgs a{};
  a.P = P;
  a.B = B;
  a.log2c = log2u(window / P);
  uint32_t n = 0;
  for (size_t i = 0; i < nrings; ++i) {
    HeatRing& R = a.r[n];
    const uint32_t first = ring(i, R);
    R.bounds = bounds + size_t(first) * B;
    R.dst = dst + size_t(first) * (P + 1) * (B + 1);
    if (++n == uint32_t(kHeatmapRingsPerLaunch) || i + 1 == nrings) {
      launch(a, n, stream);
      n = 0;
    }
  }
  return hipGetLastError();
}

}  // namespace

int launch_heatmap_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                        uint32_t P, uint32_t rows_per_col, const float* bounds, uint32_t B, int32_t* dst,
                        void* stream_ptr) {
  if (bad_columns(P) || bad_buckets(bounds, B, dst) || base == nullptr || !pow2(depth) || rows_per_col < 1 ||
      rows_per_col > kMaxTrendRowsPerColumn || depth % rows_per_col != 0 || n > depth || n > head ||
      uint64_t(n) > uint64_t(P) * rows_per_col || stride < 1 || stride > kMaxTrendStride || cols < 1 || cols > stride)
    return hipErrorInvalidValue;
  HeatArgs a{};
  a.P = P;
  a.B = B;
  a.log2c = log2u(rows_per_col);  // a divisor of a power of two
  a.r[0] = HeatRing{base, bounds, dst, head, stride, cols, depth - 1, n};
  launch(a, 1, static_cast<hipStream_t>(stream_ptr));
  return hipGetLastError();
}

// DeviceWindowSet::export_heatmap lives here with its kernel (device_window.h declares it);
// the window is export_trend's (window_trend.hip)
int DeviceWindowSet::export_heatmap(uint32_t P, const float* bounds, uint32_t B, int32_t* dst, void* stream_ptr) const {
  if (bad_columns(P) || P > window_ || window_ / P > kMaxTrendRowsPerColumn || bad_buckets(bounds, B, dst))
    return hipErrorInvalidValue;
  for (const auto& r : rings_)
    if (r.ring->width() > kMaxTrendStride) return hipErrorInvalidValue;
  DeviceScope scope(device_);
  return export_rings(rings_.size(), window_, P, bounds, B, dst, static_cast<hipStream_t>(stream_ptr),
                      [&](size_t i, HeatRing& R) {
                        const auto& r = rings_[i];
                        R.base = r.dev;
                        R.stride = R.cols = r.ring->width();
                        R.mask = uint32_t(dev_rows() - 1);
                        R.head = r.state_valid ? r.last_head : 0;
                        R.n = r.state_valid ? r.last_n : 0;
                        return r.first_series;
                      });
}

// LongWindowSet::export_heatmap: rows [copied - min(copied, W), copied), as export_trend
int LongWindowSet::export_heatmap(uint32_t P, const float* bounds, uint32_t B, int32_t* dst, void* stream_ptr) {
  if (bad_columns(P) || P > window_ || window_ / P > kMaxTrendRowsPerColumn || bad_buckets(bounds, B, dst))
    return hipErrorInvalidValue;
  if (ingest_pending_) return hipErrorNotReady;  // staged rows no kernel has written yet: refresh() first
  DeviceScope scope(device_);
  return export_rings(rings_.size(), window_, P, bounds, B, dst, static_cast<hipStream_t>(stream_ptr),
                      [&](size_t i, HeatRing& R) {
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
