// The autocorrelation's exact lag sums per trend column of a time-major device ring (see window_periods.h).
#include "window_periods.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_scope.h"
#include "device_window.h"
#include "long_window.h"
#include "window_lag_dev.h"
#include "window_periods_plan.h"

namespace rocmdash {
namespace {

using namespace lag;

constexpr int kNT = int(kThreads);  // 2 waves per SIMD, two workgroups share a CU
constexpr uint32_t kG = kPeriodsSeriesGroup;
constexpr uint32_t kLB = kPeriodsLagBlock;  // every thread owns one (series, 8 lags)
static_assert(kPeriodsChunk == kT, "the autocorrelation's chunk");
static_assert(kG == kRows && kLB % kKT == 0 && kG * (kLB / kKT) == kNT, "one item per thread");

struct PeriodsArgs {
  const float* base;        // the ring's first float
  const float* scale;       // [cols]
  unsigned long long* dst;  // [cols][P + 1][L + 1][4]; split > 1: zeroed in stream order
  uint64_t head;            // the rows are [head - n, head)
  uint32_t stride, cols, mask, n, c, P, L;  // mask: depth - 1; n <= span; c: rows of a column
  uint32_t chunks, split;                   // chunks of a full slot; workgroups that share a slot
};

// grid (slots x split, groups of kG series, blocks of kLB lags). The workgroup's slot has rows
// [b, e); it walks chunks [c0, c1) of them. Per chunk: (1) the rows [t0, t0 + len) from b - the
// chunk and the halo this block's lags reach - are read with the coalesced stream of the other
// exports (8 consecutive floats of a row per 8 lanes, rows in order, 4 loads in flight per
// lane), quantised and stored as words [series][row]; rows at and beyond e are not read and
// stored as invalid; a NaN before e marks its series. (2) a wave per series sums q per block of
// 8 words and scans the sums into pb: the exclusive prefix at every 8th word. (3) every thread
// runs its (series, 8 lags): a clean series takes n, Sx and Sy from the prefixes - all rows of
// the chunk are valid, so v[t + k] is 1 exactly while t + k is before e - and Sxy from the
// loop; a marked series takes all four from the loop. The sums of a workgroup's chunks stay in
// registers. kOwned: the workgroup has all chunks of the slot and stores every lag's four words,
// zeroes included; otherwise each non-zero sum is added to the zeroed dst with one vector atomic.
template <bool kOwned>
__global__ __launch_bounds__(kNT) void periods_ring_kernel(const PeriodsArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t w[kG * kPitch];
  __shared__ uint32_t pb[kG * kPBPitch];
  __shared__ uint32_t marked[kG];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t slot_j = kOwned ? blockIdx.x : blockIdx.x / a.split, part = kOwned ? 0u : blockIdx.x % a.split;
  const uint32_t g0 = blockIdx.y * kG, gs = min(kG, a.cols - g0);
  const uint32_t klo = blockIdx.z * kLB, khi = min(a.L, klo + kLB - 1);
  const uint32_t tiles = (khi - klo) / kKT + 1;
  const uint32_t len = (kT + khi + 16 + 7) & ~7u;  // <= kPitch
  const uint32_t nb = len >> 3;
  const bool mine = tid < gs * tiles;
  const uint32_t s = mine ? tid / tiles : 0u;
  const uint32_t k0 = klo + (mine ? tid % tiles : 0u) * kKT;
  const uint16_t* const ws = w + s * kPitch;
  const uint32_t* const pbs = pb + s * kPBPitch;
  const uint32_t col = tid & 7u;  // the loader's column: kNT is a multiple of 8
  const float sc = col < gs ? a.scale[g0 + col] : 0.f;

  uint64_t first, end;
  periods_slot(a.head, a.n, a.c, a.P, slot_j, &first, &end);  // an empty slot: N = 0, no chunk
  const uint32_t N = uint32_t(end - first);
  uint32_t cbeg, cend;
  periods_chunk_range((N + kT - 1) / kT, a.chunks, kOwned ? 1u : a.split, part, &cbeg, &cend);

  uint64_t n[kKT] = {}, sx[kKT] = {}, sy[kKT] = {}, sxy[kKT] = {};
  for (uint32_t c = cbeg; c < cend; ++c) {
    const uint32_t t0 = c * kT, left = N - t0, rows = min(kT, left);
    __syncthreads();  // the last chunk's readers are done
    if (tid < kG) marked[tid] = 0u;
    __syncthreads();
#pragma unroll 1
    for (uint32_t e0 = tid; e0 < len * 8u; e0 += kNT * 4) {
      float x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t p = (e0 + uint32_t(u) * kNT) >> 3;
        const bool in = p < len && p < left && col < gs;  // a row of the slot: ring slot < depth, column < cols
        const uint64_t rs = (first + t0 + p) & a.mask;
        x[u] = in ? a.base[rs * a.stride + g0 + col] : __builtin_nanf("");
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t p = (e0 + uint32_t(u) * kNT) >> 3;
        if (p >= len || col >= gs) continue;
        uint32_t word = kInvalid;
        if (!isnan(x[u]))
          word = uint32_t(fminf(fmaxf(rintf(x[u] * sc), 0.f), float(kAutocorrQMax)));
        else if (p < left)
          marked[col] = 1u;  // the same value from every writer
        w[col * kPitch + p] = uint16_t(word);
      }
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t r = wave; r < gs; r += kNT / 64) {
      const uint4* const row = reinterpret_cast<const uint4*>(w + r * kPitch);
      uint32_t bs[kPerLane], tot = 0;
#pragma unroll
      for (uint32_t u = 0; u < kPerLane; ++u) {
        const uint32_t j = lane * kPerLane + u;
        bs[u] = 0;
        if (j < nb) {
          const uint4 v = row[j];
          bs[u] = lo12(v.x) + hi12(v.x) + lo12(v.y) + hi12(v.y) + lo12(v.z) + hi12(v.z) + lo12(v.w) + hi12(v.w);
        }
        tot += bs[u];
      }
      uint32_t inc = tot;
#pragma unroll
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
      }
      uint32_t run = inc - tot;
#pragma unroll
      for (uint32_t u = 0; u < kPerLane; ++u) {
        const uint32_t j = lane * kPerLane + u;
        if (j <= nb) pb[r * kPBPitch + j] = run;
        run += bs[u];
      }
    }
    __syncthreads();
    if (!mine) continue;  // barriers are at the loop's head: every thread reaches them
    const uint32_t tend = (rows + 15) & ~15u;
    if (marked[s]) {
      tile<kXYandY>(ws, k0, tend, sxy, sy);
      tile<kNandX>(ws, k0, tend, n, sx);
    } else {
      tile<kXY>(ws, k0, tend, sxy, sy);
      // Sy_k = sum of q over words [k, tend + k): the words from the slot's end on are 0, and both
      // ends are j words into a block
      uint32_t ql[8], qh[8];
      unpack_q(reinterpret_cast<const uint4*>(ws + k0)[0], ql);
      unpack_q(reinterpret_cast<const uint4*>(ws + k0)[tend >> 3], qh);
      uint32_t syk = pbs[(tend + k0) >> 3] - pbs[k0 >> 3];
      const bool inner = left >= rows + k0 + kKT;  // every t + k is before the slot's end: n_k = rows
      const uint32_t whole = pbs[(rows + 7) >> 3];  // rows % 8 != 0 only in the slot's last chunk, 0 from there on
#pragma unroll
      for (uint32_t j = 0; j < kKT; ++j) {
        const uint32_t k = k0 + j;
        const uint32_t nk = k < left ? min(rows, left - k) : 0u;  // rows t of the chunk with t + k before the slot's end
        n[j] += nk;
        sx[j] += inner ? whole : prefix(ws, pbs, nk);
        sy[j] += syk;
        syk += qh[j] - ql[j];
      }
    }
  }
  if (!mine) return;
#pragma unroll
  for (uint32_t j = 0; j < kKT; ++j) {
    const uint32_t k = k0 + j;
    if (k > a.L) continue;
    unsigned long long* const d = a.dst + ((size_t(g0 + s) * (a.P + 1) + slot_j) * (a.L + 1) + k) * 4;
    if (kOwned) {  // dst is 16-byte aligned and a lag is 32 bytes
      reinterpret_cast<ulonglong2*>(d)[0] = make_ulonglong2(n[j], sx[j]);
      reinterpret_cast<ulonglong2*>(d)[1] = make_ulonglong2(sy[j], sxy[j]);
    } else {
      if (n[j]) atomicAdd(d + 0, static_cast<unsigned long long>(n[j]));
      if (sx[j]) atomicAdd(d + 1, static_cast<unsigned long long>(sx[j]));
      if (sy[j]) atomicAdd(d + 2, static_cast<unsigned long long>(sy[j]));
      if (sxy[j]) atomicAdd(d + 3, static_cast<unsigned long long>(sxy[j]));
    }
  }
}

// the newest min(n, span) rows of one ring of `depth` rows onto dst; the arguments are checked
inline int run(const float* base, uint32_t stride, uint32_t cols, uint64_t depth, uint64_t head, uint64_t n, uint32_t span,
               uint32_t P, const float* scale, uint32_t L, int64_t* dst, const PeriodsPlan& plan, hipStream_t stream) {
  PeriodsArgs a{};
  a.base = base;
  a.scale = scale;
  a.dst = reinterpret_cast<unsigned long long*>(dst);
  a.head = head;
  a.stride = stride;
  a.cols = cols;
  a.mask = uint32_t(depth - 1);
  a.n = uint32_t(std::min<uint64_t>(n, span));
  a.c = span / P;
  a.P = P;
  a.L = L;
  a.chunks = plan.chunks;
  a.split = plan.split;
  const dim3 grid((P + 1) * plan.split, plan.groups, plan.blocks);
  if (plan.split == 1) {
    hipLaunchKernelGGL(periods_ring_kernel<true>, grid, dim3(kNT), 0, stream, a);
  } else {
    const hipError_t e = hipMemsetAsync(dst, 0, size_t(cols) * (P + 1) * (L + 1) * 4 * sizeof(int64_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(periods_ring_kernel<false>, grid, dim3(kNT), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace

int launch_periods_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                        uint32_t span, uint32_t P, const float* scale, uint32_t L, int64_t* dst, uint32_t split,
                        void* stream_ptr) {
  if (bad_periods(span, P, scale, L, dst) || base == nullptr || !periods_pow2(depth) || n > depth || n > head ||
      stride < 1 || stride > kMaxAutocorrStride || cols < 1 || cols > stride)
    return hipErrorInvalidValue;
  PeriodsPlan plan;
  if (!periods_plan(P + 1, span / P, cols, L, split, &plan)) return hipErrorInvalidValue;
  return run(base, stride, cols, depth, head, n, span, P, scale, L, dst, plan, static_cast<hipStream_t>(stream_ptr));
}

// DeviceWindowSet::export_periods lives here with its kernel (device_window.h declares it); the
// window is export_trend's (window_trend.hip).
int DeviceWindowSet::export_periods(uint32_t span, uint32_t P, const float* scale, uint32_t L, int64_t* dst,
                                    void* stream_ptr) const {
  if (bad_periods(span, P, scale, L, dst) || span > window_) return hipErrorInvalidValue;
  for (const auto& r : rings_)
    if (r.ring->width() > kMaxAutocorrStride) return hipErrorInvalidValue;
  auto stream = static_cast<hipStream_t>(stream_ptr);
  DeviceScope scope(device_);
  for (const auto& r : rings_) {
    const uint32_t wd = r.ring->width();
    PeriodsPlan plan;
    if (!periods_plan(P + 1, span / P, wd, L, 0, &plan)) return hipErrorInvalidValue;
    const int err = run(r.dev, wd, wd, dev_rows(), r.state_valid ? r.last_head : 0, r.state_valid ? r.last_n : 0, span, P,
                        scale + r.first_series, L, dst + size_t(r.first_series) * (P + 1) * (L + 1) * 4, plan, stream);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

// LongWindowSet::export_periods: rows [copied - min(copied, W), copied), as export_trend
int LongWindowSet::export_periods(uint32_t span, uint32_t P, const float* scale, uint32_t L, int64_t* dst, void* stream_ptr) {
  if (bad_periods(span, P, scale, L, dst) || span > window_) return hipErrorInvalidValue;
  for (const auto& r : rings_)
    if (r.ring->width() > kMaxAutocorrStride) return hipErrorInvalidValue;
  if (ingest_pending_) return hipErrorNotReady;  // staged rows no kernel has written yet: refresh() first
  auto stream = static_cast<hipStream_t>(stream_ptr);
  DeviceScope scope(device_);
  for (const auto& r : rings_) {
    const uint32_t wd = r.ring->width();
    PeriodsPlan plan;
    if (!periods_plan(P + 1, span / P, wd, L, 0, &plan)) return hipErrorInvalidValue;
    const int err = run(r.dev.get<float>(), wd, wd, window_, r.copied, std::min<uint64_t>(r.copied, window_), span, P,
                        scale + r.first_series, L, dst + size_t(r.first_series) * (P + 1) * (L + 1) * 4, plan, stream);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace rocmdash
