// Cumulative le-bucket counts of the sorted windows (see window_buckets.h).
#include "window_buckets.h"

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_window.h"
#include "window_stats.h"
#include "window_stats_dev.h"

namespace rocmdash {
namespace {

constexpr int kWavesPerGroup = 4;  // series per workgroup: one wave64 each
constexpr int NT = 64 * kWavesPerGroup;

struct BucketRef {
  const float* sorted;       // the series' two halves of `cap` floats
  const SeriesState* state;  // written by the window-stats kernel on the same stream
  uint32_t cap;
};

struct BucketArgs {
  BucketRef s[kBucketSeriesPerLaunch];
};

// The wave's series within the launch: uniform, so a by-value argument indexed with it
// stays a kernel argument (scalar loads) instead of a per-lane copy.
__device__ __forceinline__ uint32_t wave_series() {
  return blockIdx.x * kWavesPerGroup + uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
}

// One wave over one ascending list of nv samples: lane b < B its count of samples <= bounds[b]
// (an upper_bound: ties count, -0.0 == +0.0, +inf padding past nv is never read), lane B
// the count of all; lanes past B hold 0.
__device__ __forceinline__ uint32_t bucket_count(const float* sorted, uint32_t nv, const float* bounds, uint32_t B,
                                                 uint32_t lane) {
  if (lane < B) return bound<true>(sorted, 0u, nv, bounds[lane]);
  return lane == B ? nv : 0u;
}

__global__ __launch_bounds__(NT) void export_buckets_kernel(const BucketArgs a, uint32_t n, uint32_t first, uint32_t W,
                                                           const float* __restrict__ bounds, uint32_t B,
                                                           float* __restrict__ dst) {
  const uint32_t i = wave_series();
  if (i >= n) return;
  const uint32_t lane = threadIdx.x & 63u;
  const BucketRef r = a.s[i];
  const SeriesState st = *r.state;
  const uint32_t nv = st.valid ? min(st.nvalid, min(W, r.cap)) : 0u;
  const float* src = r.sorted + size_t(st.cur & 1u) * r.cap;
  const size_t s = size_t(first) + i;
  const uint32_t c = bucket_count(src, nv, bounds + s * B, B, lane);
  if (lane <= B) dst[s * (B + 1) + lane] = float(c);
}

__global__ __launch_bounds__(NT) void bucket_blocks_kernel(const float* __restrict__ blocks, uint32_t N, uint32_t S,
                                                          uint32_t W, const float* __restrict__ bounds, uint32_t B,
                                                          float* __restrict__ per_rank, float* __restrict__ node) {
  const uint32_t s = wave_series();
  if (s >= S) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t total = 0;
  for (uint32_t i = 0; i < N; ++i) {
    const float* row = blocks + (size_t(i) * S + s) * (size_t(W) + 1);
    const float cf = row[0];
    const uint32_t nv = cf > 0.f ? min(uint32_t(cf), W) : 0u;
    const uint32_t c = bucket_count(row + 1, nv, bounds + size_t(s) * B, B, lane);
    if (per_rank != nullptr && lane <= B) per_rank[(size_t(i) * S + s) * (B + 1) + lane] = float(c);
    total += c;
  }
  if (node != nullptr && lane <= B) node[size_t(s) * (B + 1) + lane] = float(total);
}

inline uint32_t groups_for(uint32_t series) { return (series + kWavesPerGroup - 1) / kWavesPerGroup; }

}  // namespace

int launch_bucket_blocks(const float* blocks, uint32_t N, uint32_t S, uint32_t W, const float* bounds, uint32_t B,
                         float* per_rank, float* node, void* stream_ptr) {
  if (B < 1 || B > kMaxBuckets || W == 0 || N > kMaxBucketRanks || blocks == nullptr || bounds == nullptr)
    return hipErrorInvalidValue;
  if (N == 0 || S == 0 || (per_rank == nullptr && node == nullptr)) return hipSuccess;
  hipLaunchKernelGGL(bucket_blocks_kernel, dim3(groups_for(S)), dim3(NT), 0, static_cast<hipStream_t>(stream_ptr),
                     blocks, N, S, W, bounds, B, per_rank, node);
  return hipGetLastError();
}

// DeviceWindowSet::export_buckets lives here with its kernel (device_window.h declares it)
int DeviceWindowSet::export_buckets(const float* bounds, uint32_t B, float* dst, void* stream_ptr) const {
  if (B < 1 || B > kMaxBuckets || bounds == nullptr || dst == nullptr || window_ == 0) return hipErrorInvalidValue;
  auto stream = static_cast<hipStream_t>(stream_ptr);
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != device_) (void)hipSetDevice(device_);
  BucketArgs a{};
  uint32_t n = 0, first = 0;
  auto flush = [&]() {
    if (!n) return;
    hipLaunchKernelGGL(export_buckets_kernel, dim3(groups_for(n)), dim3(NT), 0, stream, a, n, first, window_, bounds, B,
                       dst);
    first += n;
    n = 0;
  };
  for (const auto& r : rings_) {
    for (uint32_t c = 0; c < r.ring->width(); ++c) {
      a.s[n++] = BucketRef{r.sorted + size_t(c) * 2 * window_, r.state + c, window_};
      if (n == uint32_t(kBucketSeriesPerLaunch)) flush();
    }
  }
  flush();
  const hipError_t e = hipGetLastError();
  if (prev >= 0 && prev != device_) (void)hipSetDevice(prev);
  return e;
}

}  // namespace rocmdash
