// Cumulative le-bucket counts streamed from the time-major device rings (see
// long_window_buckets.h).
#include "long_window_buckets.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_scope.h"
#include "long_window.h"
#include "window_buckets.h"

namespace rocmdash {
namespace {

constexpr int kNT = 512;  // 8 waves; 4 workgroups of this LDS footprint share a CU: 32 waves
constexpr int kNW = kNT / 64;
constexpr int kUnroll = 8;             // loads a lane has in flight before it bins any of them
constexpr uint32_t kMaxGroups = 1024;  // workgroups per block of rows: 4 per CU, all resident at once
constexpr int kFinalizeNT = 256;       // finalize: one wave64 per series, 4 per workgroup
constexpr int kBlocksPerLaunch = 2 * kBucketRingsPerLaunch;

// A window is one contiguous block of ring rows, or two when it wraps (its rows up to the
// ring's last slot, then those from slot 0): the blocks of one ring add onto the same bins.
struct BucketBlock {
  const float* base;    // the block's first float
  const float* bounds;  // the ring's first series' [B]
  uint32_t* bins;       // ... [B + 1] doubles: bin (c, k) is the low word of double c * (B + 1) + k
  uint64_t floats;      // rows x stride
  uint32_t stride, cols;
};

struct BucketArgs {
  BucketBlock b[kBlocksPerLaunch];  // blockIdx.y
  uint32_t B;
};

// grid (workgroups, blocks of rows). A block's floats are cut into pieces of L floats - L the
// largest multiple of the stride a wave holds, so lane l stays on series l % stride - and a
// workgroup takes a contiguous share of the pieces, its wave w runs of kUnroll consecutive
// pieces of it (w, w + kNW, ... in units of kUnroll): coalesced 4-byte loads at a uniform
// base + the lane, kUnroll of them in flight per lane.
//
// A lane bins a sample by bin = #{b : bounds[b] < x} and counts runs: it keeps the bin of its
// last sample, the bin's edges (lo, hi] and the length of the run in registers, and a sample
// inside the edges - telemetry moves slowly against the width of a bucket - only increments
// the run. A sample that left the bin flushes the run to the lane's LDS counter with one add
// and finds its bin: a guess as if the bounds were evenly spaced (the default bounds are),
// then a walk, edge by edge, over the lane's own LDS column of the bounds (conflict-free) to
// the bin that holds it - no step for evenly spaced bounds, exact for any. NaN edges stand for
// "no edge": bin 0 has no lower one, bin B no upper one.
__global__ __launch_bounds__(kNT) void bucket_ring_kernel(const BucketArgs a) {
  __shared__ float sb[(kMaxBuckets + 2) * 64];      // [k][lane]: NaN, the lane's series' bounds, NaN
  __shared__ uint32_t cnt[(kMaxBuckets + 1) * 64];  // [bin][lane], shared by the waves
  const BucketBlock& R = a.b[blockIdx.y];
  const uint32_t B = a.B, stride = R.stride;
  const uint32_t per = 64u / stride;  // lanes per series
  const uint32_t L = per * stride;
  const uint64_t F = R.floats;
  const uint32_t pieces = uint32_t((F + L - 1) / L);
  const uint32_t share = (pieces + gridDim.x - 1) / gridDim.x;
  const uint32_t pb = blockIdx.x * share;
  if (pb >= pieces) return;  // the whole workgroup, before any barrier
  const uint32_t pe = min(pb + share, pieces);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
  const float nan = __builtin_nanf("");

  for (uint32_t i = threadIdx.x; i < (B + 1) * 64u; i += kNT) cnt[i] = 0u;
  for (uint32_t i = threadIdx.x; i < (B + 2) * 64u; i += kNT) {
    const uint32_t k = i >> 6, l = i & 63u, c = l % stride;
    sb[i] = (k >= 1 && k <= B && l < L && c < R.cols) ? R.bounds[size_t(c) * B + (k - 1)] : nan;
  }
  __syncthreads();

  if (lane < L && lane % stride < R.cols) {  // columns >= cols are never read
    const float b0 = sb[64 + lane];
    const float inv = B > 1 ? float(B - 1) / (sb[B * 64 + lane] - b0) : 0.f;  // bins per unit
    uint32_t bin = 0, run = 0;
    float lo = nan, hi = b0;
    for (uint32_t k0 = pb + wave * kUnroll; k0 < pe; k0 += kNW * kUnroll) {
      float v[kUnroll];
      uint32_t have[kUnroll];  // uniform: the piece's floats (0 past the share, < L in the block's last piece)
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint32_t k = k0 + uint32_t(u);
        const uint64_t i0 = k < pe ? uint64_t(k) * L : 0;  // < F
        have[u] = k < pe ? uint32_t(min(F - i0, uint64_t(L))) : 0u;
        v[u] = R.base[i0 + (lane < have[u] ? lane : 0u)];  // every lane loads, a float of the block
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const float x = v[u];
        if (lane >= have[u] || isnan(x)) continue;
        if (x <= lo || hi < x) {
          if (run) atomicAdd(&cnt[bin * 64 + lane], run);
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
    if (run) atomicAdd(&cnt[bin * 64 + lane], run);
  }
  __syncthreads();

  // the workgroup's bin (c, k): the lanes c, c + stride, ... ; one vector atomic per non-zero bin
  for (uint32_t e = threadIdx.x; e < R.cols * (B + 1); e += kNT) {
    const uint32_t c = e / (B + 1), k = e - c * (B + 1);
    uint32_t sum = 0;
    for (uint32_t j = 0; j < per; ++j) sum += cnt[k * 64 + c + j * stride];
    if (sum) atomicAdd(&R.bins[2 * size_t(e)], sum);
  }
}

// One wave per series: lane k <= B reads bin k from the low word of double k, the wave scans,
// lane k stores the count of samples <= bounds[k] (lane B: of all) over its own bin.
__global__ __launch_bounds__(kFinalizeNT) void bucket_finalize_kernel(double* dst, uint32_t S, uint32_t B) {
  const uint32_t s = blockIdx.x * (kFinalizeNT / 64) + uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
  if (s >= S) return;  // whole waves; no barrier
  const uint32_t lane = threadIdx.x & 63u;
  double* slot = dst + size_t(s) * (B + 1) + lane;
  uint32_t c = lane <= B ? *reinterpret_cast<const uint32_t*>(slot) : 0u;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = uint32_t(__shfl_up(int(c), off));
    if (lane >= uint32_t(off)) c += o;
  }
  if (lane <= B) *slot = double(c);
}

inline bool bad_buckets(const float* bounds, uint32_t B, const double* dst) {
  return B < 1 || B > kMaxBuckets || bounds == nullptr || dst == nullptr || (reinterpret_cast<uintptr_t>(dst) & 7u) != 0;
}

// One call's launches: the blocks of every window, counted in groups of kBlocksPerLaunch.
struct BucketLaunches {
  BucketArgs a{};
  uint32_t n = 0;
  hipStream_t stream;
  BucketLaunches(uint32_t B, hipStream_t s) : stream(s) { a.B = B; }

  void flush() {
    uint64_t pieces = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t L = 64u / a.b[i].stride * a.b[i].stride;
      pieces = std::max(pieces, (a.b[i].floats + L - 1) / L);
    }
    if (n) {
      const uint32_t groups = uint32_t(std::min<uint64_t>((pieces + kNW * kUnroll - 1) / (kNW * kUnroll), kMaxGroups));
      hipLaunchKernelGGL(bucket_ring_kernel, dim3(groups, n), dim3(kNT), 0, stream, a);
    }
    n = 0;
  }
  // the window [head - n, head) of a ring of `depth` rows at `base`, onto dst's low words
  void add(const float* base, uint32_t stride, uint32_t cols, uint64_t depth, uint64_t head, uint64_t rows,
           const float* bounds, double* dst) {
    if (head == 0 || rows == 0) return;  // the zeroes stand
    if (n + 2 > uint32_t(kBlocksPerLaunch)) flush();
    const uint64_t first = (head - rows) & (depth - 1), tail = std::min(rows, depth - first);
    auto bins = reinterpret_cast<uint32_t*>(dst);
    a.b[n++] = BucketBlock{base + first * stride, bounds, bins, tail * stride, stride, cols};
    if (tail < rows) a.b[n++] = BucketBlock{base, bounds, bins, (rows - tail) * stride, stride, cols};
  }
  // zero dst [S][B + 1] first; then add() the windows; then this: the counts
  int finish(double* dst, uint32_t S) {
    flush();
    hipLaunchKernelGGL(bucket_finalize_kernel, dim3((S + kFinalizeNT / 64 - 1) / (kFinalizeNT / 64)), dim3(kFinalizeNT),
                       0, stream, dst, S, a.B);
    return hipGetLastError();
  }
};

}  // namespace

int launch_bucket_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                       const float* bounds, uint32_t B, double* dst, void* stream_ptr) {
  if (bad_buckets(bounds, B, dst) || base == nullptr || !pow2(depth) || n > depth || n > head || stride < 1 ||
      stride > kMaxBucketStride || cols < 1 || cols > stride)
    return hipErrorInvalidValue;
  auto stream = static_cast<hipStream_t>(stream_ptr);
  const hipError_t e = hipMemsetAsync(dst, 0, size_t(cols) * (B + 1) * sizeof(double), stream);
  if (e != hipSuccess) return e;
  if (n == 0) return hipSuccess;  // head >= n: not 0 either
  BucketLaunches l(B, stream);
  l.add(base, stride, cols, depth, head, n, bounds, dst);
  return l.finish(dst, cols);
}

// LongWindowSet::export_buckets lives here with its kernel (long_window.h declares it). The
// window the last refresh() left on the device: rows [copied - min(copied, W), copied), as
// in export_trend (window_trend.hip).
int LongWindowSet::export_buckets(const float* bounds, uint32_t B, double* dst, void* stream_ptr) {
  if (bad_buckets(bounds, B, dst)) return hipErrorInvalidValue;
  if (ingest_pending_) return hipErrorNotReady;  // staged rows no kernel has written yet: refresh() first
  if (nseries_ == 0) return hipSuccess;
  auto stream = static_cast<hipStream_t>(stream_ptr);
  DeviceScope scope(device_);
  const hipError_t e = hipMemsetAsync(dst, 0, size_t(nseries_) * (B + 1) * sizeof(double), stream);
  if (e != hipSuccess) return e;
  BucketLaunches l(B, stream);
  for (const auto& r : rings_)
    l.add(r.dev.get<float>(), r.ring->width(), r.ring->width(), window_, r.copied, std::min<uint64_t>(r.copied, window_),
          bounds + size_t(r.first_series) * B, dst + size_t(r.first_series) * (B + 1));
  return l.finish(dst, nseries_);
}

}  // namespace rocmdash
