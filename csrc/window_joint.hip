// Joint le-bucket counts of pairs of series, streamed from the time-major device rings (see
// window_joint.h).
#include "window_joint.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "device_scope.h"
#include "device_window.h"
#include "long_window.h"

namespace rocmdash {
namespace {

constexpr int kNT = 512;  // 8 waves; 3 workgroups of this LDS footprint share a CU: 24 waves
constexpr int kNW = kNT / 64;
constexpr int kUnroll = 8;            // loads a lane has in flight before it bins any of them
constexpr uint32_t kMaxGroups = 768;  // workgroups per block of rows: 3 per CU, all resident at once
constexpr uint32_t kMaxCells = (kMaxJointBuckets + 1) * (kMaxJointBuckets + 1);
constexpr int kMaxBlocks = 2 * int(kMaxJointPairs);  // at most 8 rings have a pair, two blocks each
constexpr int kNoBin = 0x8000;                       // a lane without a valid sample in this row

// A window is one contiguous block of ring rows, or two when it wraps (joint_cut); the blocks
// of one ring add onto the same cells.
struct JointBlock {
  const float* base;      // the block's first float
  const float* bounds;    // the ring's first series' [B]
  uint64_t floats;        // rows x stride
  uint64_t pa, pb, slots;  // JointRingPairs: columns a, b and output slots of the distinct pairs
  uint32_t stride, cols, distinct, pad;
};

struct JointArgs {
  JointBlock b[kMaxBlocks];  // blockIdx.y
  uint32_t* dst;             // [K][(B + 1)^2]
  uint32_t B;
};

// grid (workgroups, blocks of rows). The stream is bucket_ring_kernel's: a block's floats are
// cut into pieces of L floats - L the largest multiple of the stride a wave holds, so lane l
// stays on series l % stride and row l / stride of the piece - and a workgroup takes a
// contiguous share of the pieces, its wave w runs of kUnroll consecutive pieces of it:
// coalesced 4-byte loads at a uniform base + the lane, kUnroll of them in flight per lane.
//
// A lane bins its own sample as bucket_ring_kernel does: it keeps its bin and the bin's edges
// (lo, hi] in registers, and a sample that left them finds its bin by a guess as if the bounds
// were evenly spaced, then a walk over the lane's own LDS column of the bounds - exact for any
// bounds. NaN edges stand for "no edge". A lane without a valid sample (NaN, a padding column,
// past the block) carries kNoBin. Then every lane of the wave, in uniform control flow, reads
// the bins of the pair it owns (joint_owned_pair: lane c of a row owns the ring's pairs c and
// c + stride) from the two lanes of its row that hold them - a wave shuffle, no memory - and,
// when both are valid, counts the cell a x (B + 1) + b in the workgroup's LDS table
// [pair][cell] with one LDS atomic per (row, pair). Keeping the owner's last cell and a run
// length in registers and adding only when the cell changes - the bucket kernel's trick - was
// measured and is slower here (302 against 270 us on 12 series x 2^24
// telemetry-like rows), so it is not done.
__global__ __launch_bounds__(kNT) void joint_ring_kernel(const JointArgs a) {
  __shared__ float sb[(kMaxJointBuckets + 2) * 64];        // [k][lane]: NaN, the lane's series' bounds, NaN
  __shared__ uint32_t tab[kMaxJointPairs * kMaxCells];     // [distinct pair][cell], shared by the waves
  const uint32_t blk = blockIdx.y;
  const float* const base = a.b[blk].base;
  const float* const bounds = a.b[blk].bounds;
  const uint64_t F = a.b[blk].floats, pa = a.b[blk].pa, pb = a.b[blk].pb, slots = a.b[blk].slots;
  const uint32_t stride = a.b[blk].stride, cols = a.b[blk].cols, U = a.b[blk].distinct;
  const uint32_t B = a.B, B1 = B + 1, cells = B1 * B1;
  const uint32_t L = joint_piece_floats(stride);
  const uint32_t pieces = joint_pieces(F, stride);
  const uint32_t share = joint_share(pieces, gridDim.x);
  const uint32_t pb0 = blockIdx.x * share;
  if (pb0 >= pieces) return;  // the whole workgroup, before any barrier
  const uint32_t pe = min(pb0 + share, pieces);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
  const float nan = __builtin_nanf("");

  for (uint32_t i = threadIdx.x; i < U * cells; i += kNT) tab[i] = 0u;
  for (uint32_t i = threadIdx.x; i < (B + 2) * 64u; i += kNT) {
    const uint32_t k = i >> 6, l = i & 63u, c = l % stride;
    sb[i] = (k >= 1 && k <= B && l < L && c < cols) ? bounds[size_t(c) * B + (k - 1)] : nan;
  }
  __syncthreads();

  const uint32_t c = lane % stride, row0 = lane - c;  // the lane's column, its row's first lane
  const bool series = lane < L && c < cols;           // columns >= cols are never binned
  // the pairs this lane owns, one per pass; a lane that owns none shuffles with itself
  const int q0 = lane < L ? joint_owned_pair(stride, U, c, 0) : -1;
  const int q1 = lane < L ? joint_owned_pair(stride, U, c, 1) : -1;
  const bool two = U > stride;  // uniform: some lane owns a second pair
  const int a0 = int(q0 >= 0 ? row0 + joint_byte(pa, uint32_t(q0)) : lane);
  const int b0 = int(q0 >= 0 ? row0 + joint_byte(pb, uint32_t(q0)) : lane);
  const int a1 = int(q1 >= 0 ? row0 + joint_byte(pa, uint32_t(q1)) : lane);
  const int b1 = int(q1 >= 0 ? row0 + joint_byte(pb, uint32_t(q1)) : lane);
  uint32_t* const t0 = tab + uint32_t(q0 >= 0 ? q0 : 0) * cells;
  uint32_t* const t1 = tab + uint32_t(q1 >= 0 ? q1 : 0) * cells;

  const float e0 = sb[64 + lane];
  const float inv = B > 1 ? float(B - 1) / (sb[B * 64 + lane] - e0) : 0.f;  // bins per unit
  uint32_t bin = 0;
  float lo = nan, hi = e0;
  for (uint32_t k0 = pb0 + wave * kUnroll; k0 < pe; k0 += kNW * kUnroll) {
    float v[kUnroll];
    uint32_t have[kUnroll];  // uniform: the piece's floats (0 past the share, < L in the block's last piece)
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint32_t k = k0 + uint32_t(u);
      const uint64_t i0 = k < pe ? uint64_t(k) * L : 0;  // < F
      have[u] = k < pe ? uint32_t(min(F - i0, uint64_t(L))) : 0u;
      v[u] = base[i0 + (lane < have[u] ? lane : 0u)];  // every lane loads, a float of the block
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const float x = v[u];
      const bool ok = series && lane < have[u] && !isnan(x);
      if (ok && (x <= lo || hi < x)) {
        // ceil((x - e0) x bins per unit) into [0, B]; inf and NaN (inf x 0) clamp too
        uint32_t g = uint32_t(fminf(fmaxf(ceilf((x - e0) * inv), 0.f), float(B)));
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
      const int mine = ok ? int(bin) : kNoBin;
      // every lane of the wave is here: the shuffles read lanes of the reader's own row
      {
        const int ba = __shfl(mine, a0), bb = __shfl(mine, b0);
        if (q0 >= 0 && !((ba | bb) & kNoBin)) {
          atomicAdd(&t0[uint32_t(ba) * B1 + uint32_t(bb)], 1u);
        }
      }
      if (two) {
        const int ba = __shfl(mine, a1), bb = __shfl(mine, b1);
        if (q1 >= 0 && !((ba | bb) & kNoBin)) {
          atomicAdd(&t1[uint32_t(ba) * B1 + uint32_t(bb)], 1u);
        }
      }
    }
  }
  __syncthreads();

  // the workgroup's non-zero cells: one vector atomic per cell and output slot that asked for the pair
  for (uint32_t e = threadIdx.x; e < U * cells; e += kNT) {
    const uint32_t sum = tab[e];
    if (!sum) continue;
    const uint32_t q = e / cells, cell = e - q * cells;
    for (uint32_t m = joint_byte(slots, q); m; m &= m - 1)
      atomicAdd(&a.dst[uint32_t(__builtin_ctz(m)) * cells + cell], sum);
  }
}

inline bool bad_joint(uint32_t K, const float* bounds, uint32_t B, const int32_t* dst) {
  return K < 1 || K > kMaxJointPairs || B < 1 || B > kMaxJointBuckets || bounds == nullptr || dst == nullptr ||
         (reinterpret_cast<uintptr_t>(dst) & 3u) != 0;
}

// One call: the blocks of every ring that has a pair, in one launch.
struct JointLaunch {
  JointArgs a{};
  uint32_t n = 0;
  // the window [head - rows, head) of a ring of `depth` rows at `base`
  void add(const JointRingPairs& p, const float* base, uint32_t stride, uint32_t cols, uint64_t depth, uint64_t head,
           uint64_t rows, const float* bounds) {
    if (head == 0 || rows == 0) return;  // the zeroes stand
    const JointCut cut = joint_cut(depth, head, rows);
    a.b[n++] = JointBlock{base + cut.first * stride, bounds, cut.tail * stride, p.a, p.b, p.slots, stride, cols, p.distinct, 0};
    if (cut.rest) a.b[n++] = JointBlock{base, bounds, cut.rest * stride, p.a, p.b, p.slots, stride, cols, p.distinct, 0};
  }
  int run(hipStream_t stream) {
    if (n == 0) return hipSuccess;
    uint64_t pieces = 0;
    for (uint32_t i = 0; i < n; ++i) pieces = std::max<uint64_t>(pieces, joint_pieces(a.b[i].floats, a.b[i].stride));
    const uint32_t groups = uint32_t(std::min<uint64_t>((pieces + kNW * kUnroll - 1) / (kNW * kUnroll), kMaxGroups));
    hipLaunchKernelGGL(joint_ring_kernel, dim3(groups, n), dim3(kNT), 0, stream, a);
    return hipGetLastError();
  }
};

inline hipError_t zero(int32_t* dst, uint32_t K, uint32_t B, hipStream_t stream) {
  return hipMemsetAsync(dst, 0, size_t(K) * (B + 1) * (B + 1) * sizeof(int32_t), stream);
}

}  // namespace

int launch_joint_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                      const uint32_t* pairs, uint32_t K, const float* bounds, uint32_t B, int32_t* dst, void* stream_ptr) {
  if (bad_joint(K, bounds, B, dst) || base == nullptr || !pow2(depth) || n > depth || n > head || stride < 1 ||
      stride > kMaxJointStride || cols < 1 || cols > stride)
    return hipErrorInvalidValue;
  const JointRingSpan span{0, cols};
  JointPlan plan;
  if (!joint_plan_pairs(pairs, K, &span, 1, &plan)) return hipErrorInvalidValue;
  auto stream = static_cast<hipStream_t>(stream_ptr);
  const hipError_t e = zero(dst, K, B, stream);
  if (e != hipSuccess) return e;
  JointLaunch l;
  l.a.dst = reinterpret_cast<uint32_t*>(dst);
  l.a.B = B;
  l.add(plan.rings[0], base, stride, cols, depth, head, n, bounds);
  return l.run(stream);
}

// DeviceWindowSet::export_joint lives here with its kernel (device_window.h declares it); the
// window is export_trend's (window_trend.hip). A ring without a pair is not streamed.
int DeviceWindowSet::export_joint(const uint32_t* pairs, uint32_t K, const float* bounds, uint32_t B, int32_t* dst,
                                  void* stream_ptr) const {
  if (bad_joint(K, bounds, B, dst)) return hipErrorInvalidValue;
  std::vector<JointRingSpan> spans;
  for (const auto& r : rings_) spans.push_back(JointRingSpan{r.first_series, r.ring->width()});
  JointPlan plan;
  if (!joint_plan_pairs(pairs, K, spans.data(), uint32_t(spans.size()), &plan)) return hipErrorInvalidValue;
  auto stream = static_cast<hipStream_t>(stream_ptr);
  DeviceScope scope(device_);
  const hipError_t e = zero(dst, K, B, stream);
  if (e != hipSuccess) return e;
  JointLaunch l;
  l.a.dst = reinterpret_cast<uint32_t*>(dst);
  l.a.B = B;
  for (uint32_t i = 0; i < plan.nrings; ++i) {
    const auto& r = rings_[plan.rings[i].ring];
    const uint32_t w = r.ring->width();
    l.add(plan.rings[i], r.dev, w, w, dev_rows(), r.state_valid ? r.last_head : 0, r.state_valid ? r.last_n : 0,
          bounds + size_t(r.first_series) * B);
  }
  return l.run(stream);
}

// LongWindowSet::export_joint: rows [copied - min(copied, W), copied), as export_buckets
int LongWindowSet::export_joint(const uint32_t* pairs, uint32_t K, const float* bounds, uint32_t B, int32_t* dst,
                                void* stream_ptr) {
  if (bad_joint(K, bounds, B, dst)) return hipErrorInvalidValue;
  std::vector<JointRingSpan> spans;
  for (const auto& r : rings_) spans.push_back(JointRingSpan{r.first_series, r.ring->width()});
  JointPlan plan;
  if (!joint_plan_pairs(pairs, K, spans.data(), uint32_t(spans.size()), &plan)) return hipErrorInvalidValue;
  if (ingest_pending_) return hipErrorNotReady;  // staged rows no kernel has written yet: refresh() first
  auto stream = static_cast<hipStream_t>(stream_ptr);
  DeviceScope scope(device_);
  const hipError_t e = zero(dst, K, B, stream);
  if (e != hipSuccess) return e;
  JointLaunch l;
  l.a.dst = reinterpret_cast<uint32_t*>(dst);
  l.a.B = B;
  for (uint32_t i = 0; i < plan.nrings; ++i) {
    const auto& r = rings_[plan.rings[i].ring];
    const uint32_t w = r.ring->width();
    l.add(plan.rings[i], r.dev.get<float>(), w, w, window_, r.copied, std::min<uint64_t>(r.copied, window_),
          bounds + size_t(r.first_series) * B);
  }
  return l.run(stream);
}

}  // namespace rocmdash
