// Episodes above a threshold, counted in time order over the time-major device rings (see
// window_excursions.h).
#include "window_excursions.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_scope.h"
#include "device_window.h"
#include "long_window.h"
#include "window_excursions_monoid.h"

namespace rocmdash {
namespace {

constexpr int kNT = 256;  // 4 waves; 4 workgroups per CU hold 1024 chunks at once
constexpr int kNW = kNT / 64;
constexpr int kUnroll = 8;        // loads a lane has in flight before it folds any of them
constexpr int kFinalizeNT = 256;  // finalize: one wave64 per (series, threshold), 4 per workgroup
constexpr int kFinalizeUnroll = 4;

struct ExcRing {
  const float* base;  // device ring: slot s at base + s * stride
  const float* thr;   // the ring's first series' [K]
  uint4* work;        // the ring's partials: [chunk][col][K] of 2 x uint4
  int32_t* dst;       // the ring's first series' [K][8]
  uint32_t stride, cols;
  uint32_t first;       // slot of the window's oldest row: block 0 starts there, block 1 at slot 0
  uint32_t rows0, n;    // rows of block 0, of the window
  uint32_t chunk_rows;  // >= 1
  uint32_t chunks0, chunks;  // chunks of block 0, of both blocks (block 0's first)
};

struct ExcArgs {
  ExcRing r[kExcursionRingsPerLaunch];  // blockIdx.y
};

__device__ __forceinline__ ExcursionPartial shfl_partial(const ExcursionPartial& p, int src) {
  ExcursionPartial o;
  o.len = uint32_t(__shfl(int(p.len), src));
  o.above = uint32_t(__shfl(int(p.above), src));
  o.pre = uint32_t(__shfl(int(p.pre), src));
  o.suf = uint32_t(__shfl(int(p.suf), src));
  o.longest = uint32_t(__shfl(int(p.longest), src));
  o.episodes = uint32_t(__shfl(int(p.episodes), src));
  o.tail_below = uint32_t(__shfl(int(p.tail_below), src));
  return o;
}

// grid (chunks, rings). Chunk j of a ring is rows [cb, ce) of one of the window's blocks; wave
// w takes the w-th quarter of them and, with per = 64 / stride lanes per series, lane
// (i, c) = (lane / stride, lane % stride) the i-th share of the wave's rows, consecutive, of
// series c - not the rows i, i + per, ... of the order-free streams: a run length needs its
// samples in order. The lanes of one i read one row's floats together and every lane walks
// forward row by row, so a cache line a wave touches is used up within a few iterations;
// kUnroll rows are in flight per lane. Rows past a lane's share load as NaN, which the
// monoid skips.
template <int K>
__global__ __launch_bounds__(kNT) void excursion_stream_kernel(const ExcArgs a) {
  __shared__ ExcursionPartial sh[kNW][K][kMaxExcursionStride];
  const ExcRing& R = a.r[blockIdx.y];
  const uint32_t j = blockIdx.x;
  if (j >= R.chunks) return;  // the whole workgroup, before any barrier
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
  const uint32_t stride = R.stride;

  const bool second = j >= R.chunks0;
  const uint32_t brows = second ? R.n - R.rows0 : R.rows0;
  const float* p = R.base + (second ? size_t(0) : size_t(R.first) * stride);  // the block's first float
  const uint32_t cb = (second ? j - R.chunks0 : j) * R.chunk_rows;            // < brows
  const uint32_t ce = cb + min(R.chunk_rows, brows - cb);
  const uint32_t wrows = (ce - cb + kNW - 1) / kNW;
  const uint32_t wb = min(cb + wave * wrows, ce), we = wb + min(wrows, ce - wb);

  const uint32_t per = 64u / stride;  // lanes per series
  const uint32_t c = lane % stride, i = lane / stride;
  const bool active = i < per && c < R.cols;  // columns >= cols are never read
  const uint32_t lrows = (we - wb + per - 1) / per;
  const uint32_t lb = min(wb + i * lrows, we);
  const uint32_t le = active ? lb + min(lrows, we - lb) : lb;

  float t[K];
#pragma unroll
  for (int k = 0; k < K; ++k) t[k] = active ? R.thr[size_t(c) * K + k] : 0.f;

  ExcursionPartial acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = ExcursionPartial{0, 0, 0, 0, 0, 0, 0};
  for (uint32_t r = lb; r < le; r += kUnroll) {
    float v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      v[u] = r + uint32_t(u) < le ? p[size_t(r + uint32_t(u)) * stride + c] : __builtin_nanf("");
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const float x = v[u];
      const bool valid = !isnan(x);
#pragma unroll
      for (int k = 0; k < K; ++k) excursion_push(acc[k], valid, x > t[k]);
    }
  }

  // the series' lanes c, c + stride, ... hold consecutive time ranges: an ordered tree over
  // their index i, [i, i + off) then [i + off, i + 2 off), leaves the wave's partial in i == 0
  for (uint32_t off = 1; off < per; off <<= 1) {
    const int src = int(lane + off * stride) & 63;
    const bool take = i < per && (i & (2 * off - 1)) == 0 && i + off < per;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const ExcursionPartial o = shfl_partial(acc[k], src);
      if (take) acc[k] = excursion_combine(acc[k], o);
    }
  }
  if (lane < R.cols) {  // i == 0
#pragma unroll
    for (int k = 0; k < K; ++k) sh[wave][k][lane] = acc[k];
  }
  __syncthreads();

  // the waves in wave order; one partial per (chunk, series, threshold)
  const uint32_t e = threadIdx.x;
  if (e < R.cols * uint32_t(K)) {
    const uint32_t col = e / uint32_t(K), k = e % uint32_t(K);
    ExcursionPartial s = sh[0][k][col];
    for (int w = 1; w < kNW; ++w) s = excursion_combine(s, sh[w][k][col]);
    uint4* out = R.work + (size_t(j) * R.cols * K + e) * 2;
    out[0] = uint4{s.len, s.above, s.pre, s.suf};
    out[1] = uint4{s.longest, s.episodes, s.tail_below, 0u};
  }
}

// grid (ceil(cols x K / 4), rings): one wave per (series, threshold). Lane l folds the chunks
// [l q, (l + 1) q), q = ceil(chunks / 64) <= 16, in order; the 64 lanes combine in the same
// ordered tree; lane 0 writes the record. chunks == 0 (an empty window) gives the identity:
// all zeroes.
__global__ __launch_bounds__(kFinalizeNT) void excursion_finalize_kernel(const ExcArgs a, uint32_t K) {
  const ExcRing& R = a.r[blockIdx.y];
  const uint32_t e = blockIdx.x * (kFinalizeNT / 64) + uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
  if (e >= R.cols * K) return;  // whole waves; no barrier
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = (R.chunks + 63u) / 64u;
  const uint32_t jb = min(lane * q, R.chunks), je = min(jb + q, R.chunks);
  const size_t step = size_t(R.cols) * K * 2;
  const uint4* w = R.work + size_t(e) * 2;

  ExcursionPartial acc{0, 0, 0, 0, 0, 0, 0};
  for (uint32_t j = jb; j < je; j += kFinalizeUnroll) {
    uint4 lo[kFinalizeUnroll], hi[kFinalizeUnroll];
#pragma unroll
    for (int u = 0; u < kFinalizeUnroll; ++u) {
      const bool in = j + uint32_t(u) < je;
      lo[u] = in ? w[size_t(j + uint32_t(u)) * step] : uint4{0u, 0u, 0u, 0u};
      hi[u] = in ? w[size_t(j + uint32_t(u)) * step + 1] : uint4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < kFinalizeUnroll; ++u)
      acc = excursion_combine(acc, ExcursionPartial{lo[u].x, lo[u].y, lo[u].z, lo[u].w, hi[u].x, hi[u].y, hi[u].z});
  }
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const ExcursionPartial o = shfl_partial(acc, int(lane + off) & 63);
    if ((lane & (2 * off - 1)) == 0) acc = excursion_combine(acc, o);
  }
  if (lane == 0) {
    int32_t rec[8];
    excursion_record(acc, R.n, rec);
    int4* out = reinterpret_cast<int4*>(R.dst + size_t(e) * kExcursionFields);
    out[0] = int4{rec[0], rec[1], rec[2], rec[3]};
    out[1] = int4{rec[4], rec[5], rec[6], rec[7]};
  }
}

inline bool misaligned(const void* p, uintptr_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool bad_buffers(const float* thr, uint32_t K, const int32_t* dst, const void* work, size_t work_bytes,
                        uint32_t series) {
  return K < 1 || K > kMaxExcursionThresholds || misaligned(thr, 4) || misaligned(dst, 16) || misaligned(work, 16) ||
         work_bytes < excursion_workspace_bytes(series, K);
}

// One call's launches: rings in groups of kExcursionRingsPerLaunch, stream then finalize.
struct ExcLaunches {
  ExcArgs a{};
  uint32_t n = 0, K;
  hipStream_t stream;
  ExcLaunches(uint32_t k, hipStream_t s) : K(k), stream(s) {}

  void flush() {
    if (n == 0) return;
    uint32_t chunks = 0, cols = 0;
    for (uint32_t i = 0; i < n; ++i) {
      chunks = std::max(chunks, a.r[i].chunks);
      cols = std::max(cols, a.r[i].cols);
    }
    if (chunks) {
      const dim3 grid(chunks, n), block(kNT);
      switch (K) {
        case 1: hipLaunchKernelGGL(excursion_stream_kernel<1>, grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL(excursion_stream_kernel<2>, grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL(excursion_stream_kernel<3>, grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL(excursion_stream_kernel<4>, grid, block, 0, stream, a); break;
      }
    }
    constexpr uint32_t kPer = kFinalizeNT / 64;
    hipLaunchKernelGGL(excursion_finalize_kernel, dim3((cols * K + kPer - 1) / kPer, n), dim3(kFinalizeNT), 0, stream, a, K);
    n = 0;
  }
  // the window [head - rows, head) of a ring of `depth` rows; chunk_rows >= 1 and the chunk
  // count checked by the caller. thr / dst / work: the ring's first series'.
  void add(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t rows,
           uint32_t chunk_rows, const float* thr, int32_t* dst, uint4* work) {
    ExcRing& R = a.r[n++];
    R = ExcRing{base, thr, work, dst, stride, cols, 0u, 0u, rows, chunk_rows, 0u, 0u};
    if (rows) {
      R.first = uint32_t((head - rows) & uint64_t(depth - 1));
      R.rows0 = std::min(rows, depth - R.first);
      R.chunks0 = (R.rows0 + chunk_rows - 1) / chunk_rows;
      R.chunks = R.chunks0 + (rows - R.rows0 + chunk_rows - 1) / chunk_rows;
    }
    if (n == uint32_t(kExcursionRingsPerLaunch)) flush();
  }
  int finish() {
    flush();
    return hipGetLastError();
  }
};

// the workspace of the series from `first_series` on, within a set's
inline uint4* work_of(void* work, uint32_t first_series, uint32_t K) {
  return static_cast<uint4*>(work) + size_t(first_series) * K * kMaxExcursionChunks * 2;
}

}  // namespace

size_t excursion_workspace_bytes(uint32_t series, uint32_t K) {
  if (K < 1 || K > kMaxExcursionThresholds) return 0;
  return size_t(series) * K * kMaxExcursionChunks * 2 * sizeof(uint4);
}

uint32_t excursion_plan_chunk_rows(uint32_t n) {
  return std::max(kMinExcursionChunkRows, (n + kMaxExcursionChunks - 2) / (kMaxExcursionChunks - 1));
}

uint64_t excursion_chunk_count(uint32_t depth, uint64_t head, uint32_t n, uint32_t chunk_rows) {
  if (n == 0 || chunk_rows == 0 || depth == 0) return 0;
  const uint64_t first = (head - n) & uint64_t(depth - 1), rows0 = std::min<uint64_t>(n, depth - first);
  return (rows0 + chunk_rows - 1) / chunk_rows + (n - rows0 + chunk_rows - 1) / chunk_rows;
}

int launch_excursion_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                          const float* thresholds, uint32_t K, uint32_t chunk_rows, int32_t* dst, void* work,
                          size_t work_bytes, void* stream_ptr) {
  if (stride < 1 || stride > kMaxExcursionStride || cols < 1 || cols > stride || misaligned(base, 4) || !pow2(depth) ||
      n > depth || n > head || bad_buffers(thresholds, K, dst, work, work_bytes, stride))
    return hipErrorInvalidValue;
  if (chunk_rows == 0) chunk_rows = excursion_plan_chunk_rows(n);
  chunk_rows = std::min(chunk_rows, std::max(n, 1u));  // one chunk per block at the most
  if (excursion_chunk_count(depth, head, n, chunk_rows) > kMaxExcursionChunks) return hipErrorInvalidValue;
  ExcLaunches l(K, static_cast<hipStream_t>(stream_ptr));
  l.add(base, stride, cols, depth, head, n, chunk_rows, thresholds, dst, static_cast<uint4*>(work));
  return l.finish();
}

// DeviceWindowSet::export_excursions lives here with its kernel (device_window.h declares
// it): the ring facts of export_trend (window_trend.hip).
int DeviceWindowSet::export_excursions(const float* thresholds, uint32_t K, int32_t* dst, void* work, size_t work_bytes,
                                       void* stream_ptr) const {
  if (bad_buffers(thresholds, K, dst, work, work_bytes, nseries_)) return hipErrorInvalidValue;
  for (const auto& r : rings_)
    if (r.ring->width() > kMaxExcursionStride) return hipErrorInvalidValue;
  DeviceScope scope(device_);
  ExcLaunches l(K, static_cast<hipStream_t>(stream_ptr));
  for (const auto& r : rings_) {
    const uint32_t n = r.state_valid ? r.last_n : 0;
    l.add(r.dev, r.ring->width(), r.ring->width(), uint32_t(dev_rows()), r.state_valid ? r.last_head : 0, n,
          excursion_plan_chunk_rows(n), thresholds + size_t(r.first_series) * K,
          dst + size_t(r.first_series) * K * kExcursionFields, work_of(work, r.first_series, K));
  }
  return l.finish();
}

// LongWindowSet::export_excursions: the window the last refresh() left on the device, rows
// [copied - min(copied, W), copied), as in export_trend (window_trend.hip).
int LongWindowSet::export_excursions(const float* thresholds, uint32_t K, int32_t* dst, void* work, size_t work_bytes,
                                     void* stream_ptr) {
  if (bad_buffers(thresholds, K, dst, work, work_bytes, nseries_)) return hipErrorInvalidValue;
  for (const auto& r : rings_)
    if (r.ring->width() > kMaxExcursionStride) return hipErrorInvalidValue;
  if (ingest_pending_) return hipErrorNotReady;  // staged rows no kernel has written yet: refresh() first
  DeviceScope scope(device_);
  ExcLaunches l(K, static_cast<hipStream_t>(stream_ptr));
  for (const auto& r : rings_) {
    const uint32_t n = uint32_t(std::min<uint64_t>(r.copied, window_));
    l.add(r.dev.get<float>(), r.ring->width(), r.ring->width(), window_, r.copied, n, excursion_plan_chunk_rows(n),
          thresholds + size_t(r.first_series) * K, dst + size_t(r.first_series) * K * kExcursionFields,
          work_of(work, r.first_series, K));
  }
  return l.finish();
}

}  // namespace rocmdash
