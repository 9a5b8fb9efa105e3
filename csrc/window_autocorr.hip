// Exact integer lag sums of every series of a time-major device ring (see window_autocorr.h).
#include "window_autocorr.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_scope.h"
#include "device_window.h"
#include "long_window.h"
#include "window_lag_dev.h"

namespace rocmdash {
namespace {

using namespace lag;

constexpr int kNT = int(kThreads);  // 184 VGPRs: 2 waves per SIMD, two workgroups share a CU
constexpr uint32_t kG = 8;          // series of a workgroup
constexpr uint32_t kLB = 256;       // lags of a workgroup: every thread owns one (series, 8 lags)
constexpr uint32_t kTargetGroups = 1024;  // workgroups of a launch: two rounds of 2 per CU
static_assert(kG == kRows && kLB % kKT == 0 && kG * (kLB / kKT) == kNT, "one item per thread");

struct AutocorrArgs {
  const float* base;        // the ring's first float
  const float* scale;       // [cols]
  unsigned long long* dst;  // [cols][L + 1][4], zeroed in stream order
  uint64_t first;           // the span's oldest row: head - N
  uint32_t stride, cols, mask, N, L, chunks, share;  // mask: depth - 1; share: chunks of a workgroup
};

// grid (shares of chunks, groups of kG series, blocks of kLB lags). Per chunk: (1) the rows
// [t0, t0 + len) of the span - the chunk and the halo this block's lags reach - are read with
// the coalesced stream of the other exports (8 consecutive floats of a row per 8 lanes, rows in
// order, 4 loads in flight per lane), quantised and stored as words [series][row]; rows past the
// span are stored as invalid; a NaN marks its series. (2) a wave per series sums q per block of
// 8 words and scans the sums into pb: the exclusive prefix at every 8th word. (3) every thread
// runs its (series, 8 lags): a clean series takes n, Sx and Sy from the prefixes - all rows of
// the chunk are valid, so v[t + k] is 1 exactly while t + k is in the span - and Sxy from the
// loop; a marked series takes all four from the loop. The sums of a workgroup's chunks stay in
// registers; at the end each non-zero one is added to dst with one vector atomic.
__global__ __launch_bounds__(kNT) void autocorr_ring_kernel(const AutocorrArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t w[kG * kPitch];
  __shared__ uint32_t pb[kG * kPBPitch];
  __shared__ uint32_t marked[kG];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t g0 = blockIdx.y * kG, gs = min(kG, a.cols - g0);
  const uint32_t klo = blockIdx.z * kLB, khi = min(a.L, klo + kLB - 1);
  const uint32_t tiles = (khi - klo) / kKT + 1;
  const uint32_t len = (kT + khi + 16 + 7) & ~7u;  // <= kPitch
  const uint32_t nb = len >> 3;
  const uint32_t c1 = min((blockIdx.x + 1) * a.share, a.chunks);
  const bool mine = tid < gs * tiles;
  const uint32_t s = mine ? tid / tiles : 0u;
  const uint32_t k0 = klo + (mine ? tid % tiles : 0u) * kKT;
  const uint16_t* const ws = w + s * kPitch;
  const uint32_t* const pbs = pb + s * kPBPitch;
  const uint32_t col = tid & 7u;  // the loader's column: kNT is a multiple of 8
  const float sc = col < gs ? a.scale[g0 + col] : 0.f;

  uint64_t n[kKT] = {}, sx[kKT] = {}, sy[kKT] = {}, sxy[kKT] = {};
  for (uint32_t c = blockIdx.x * a.share; c < c1; ++c) {
    const uint32_t t0 = c * kT, left = a.N - t0, rows = min(kT, left);
    __syncthreads();  // the last chunk's readers are done
    if (tid < kG) marked[tid] = 0u;
    __syncthreads();
#pragma unroll 1
    for (uint32_t e0 = tid; e0 < len * 8u; e0 += kNT * 4) {
      float x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t p = (e0 + uint32_t(u) * kNT) >> 3;
        const bool in = p < len && p < left && col < gs;  // a row of the span: slot < depth, column < cols
        const uint64_t slot = (a.first + t0 + p) & a.mask;
        x[u] = in ? a.base[slot * a.stride + g0 + col] : __builtin_nanf("");
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
      // Sy_k = sum of q over words [k, tend + k): the words from the span's end on are 0, and both
      // ends are j words into a block
      uint32_t ql[8], qh[8];
      unpack_q(reinterpret_cast<const uint4*>(ws + k0)[0], ql);
      unpack_q(reinterpret_cast<const uint4*>(ws + k0)[tend >> 3], qh);
      uint32_t syk = pbs[(tend + k0) >> 3] - pbs[k0 >> 3];
      const bool inner = left >= rows + k0 + kKT;  // every t + k is in the span: n_k = rows
      const uint32_t whole = pbs[(rows + 7) >> 3];  // rows % 8 != 0 only in the span's last chunk, 0 from there on
#pragma unroll
      for (uint32_t j = 0; j < kKT; ++j) {
        const uint32_t k = k0 + j;
        const uint32_t nk = k < left ? min(rows, left - k) : 0u;  // rows t of the chunk with t + k in the span
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
    unsigned long long* const d = a.dst + (size_t(g0 + s) * (a.L + 1) + k) * 4;
    if (n[j]) atomicAdd(d + 0, static_cast<unsigned long long>(n[j]));
    if (sx[j]) atomicAdd(d + 1, static_cast<unsigned long long>(sx[j]));
    if (sy[j]) atomicAdd(d + 2, static_cast<unsigned long long>(sy[j]));
    if (sxy[j]) atomicAdd(d + 3, static_cast<unsigned long long>(sxy[j]));
  }
}

// the span [head - min(n, span), head) of one ring of `depth` rows onto dst (already zeroed);
// share 0: the rule below, else the chunks of a workgroup, checked by the caller
inline int run(const float* base, uint32_t stride, uint32_t cols, uint64_t depth, uint64_t head, uint64_t n, uint32_t span,
               const float* scale, uint32_t L, int64_t* dst, hipStream_t stream, uint32_t share = 0) {
  const uint32_t N = uint32_t(std::min<uint64_t>(n, span));
  if (head == 0 || N == 0) return hipSuccess;  // the zeroes stand
  AutocorrArgs a{};
  a.base = base;
  a.scale = scale;
  a.dst = reinterpret_cast<unsigned long long*>(dst);
  a.first = head - N;
  a.stride = stride;
  a.cols = cols;
  a.mask = uint32_t(depth - 1);
  a.N = N;
  a.L = L;
  a.chunks = (N + kT - 1) / kT;
  // lags 0 .. L: L = 256 m - 1 fills its blocks; at L = 256 m the last block holds lag L alone
  const uint32_t groups = (cols + kG - 1) / kG, blocks = L / kLB + 1;
  const uint32_t shares = std::min(a.chunks, std::max(1u, kTargetGroups / (groups * blocks)));
  a.share = share ? share : (a.chunks + shares - 1) / shares;
  hipLaunchKernelGGL(autocorr_ring_kernel, dim3((a.chunks + a.share - 1) / a.share, groups, blocks), dim3(kNT), 0, stream, a);
  return hipGetLastError();
}

inline hipError_t zero(int64_t* dst, uint32_t S, uint32_t L, hipStream_t stream) {
  return hipMemsetAsync(dst, 0, size_t(S) * (L + 1) * 4 * sizeof(int64_t), stream);
}

}  // namespace

int launch_autocorr_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                         uint32_t span, const float* scale, uint32_t L, int64_t* dst, void* stream_ptr, uint32_t share) {
  if (bad_autocorr(span, scale, L, dst) || base == nullptr || !pow2(depth) || n > depth || n > head || stride < 1 ||
      stride > kMaxAutocorrStride || cols < 1 || cols > stride)
    return hipErrorInvalidValue;
  if (share > std::max(1u, (std::min(n, span) + kT - 1) / kT)) return hipErrorInvalidValue;  // 0: the rule
  auto stream = static_cast<hipStream_t>(stream_ptr);
  const hipError_t e = zero(dst, cols, L, stream);
  if (e != hipSuccess) return e;
  return run(base, stride, cols, depth, head, n, span, scale, L, dst, stream, share);
}

// DeviceWindowSet::export_autocorr lives here with its kernel (device_window.h declares it); the
// window is export_trend's (window_trend.hip).
int DeviceWindowSet::export_autocorr(uint32_t span, const float* scale, uint32_t L, int64_t* dst, void* stream_ptr) const {
  if (bad_autocorr(span, scale, L, dst)) return hipErrorInvalidValue;
  for (const auto& r : rings_)
    if (r.ring->width() > kMaxAutocorrStride) return hipErrorInvalidValue;
  auto stream = static_cast<hipStream_t>(stream_ptr);
  DeviceScope scope(device_);
  const hipError_t e = zero(dst, nseries_, L, stream);
  if (e != hipSuccess) return e;
  for (const auto& r : rings_) {
    const uint32_t wd = r.ring->width();
    const int err = run(r.dev, wd, wd, dev_rows(), r.state_valid ? r.last_head : 0, r.state_valid ? r.last_n : 0, span,
                        scale + r.first_series, L, dst + size_t(r.first_series) * (L + 1) * 4, stream);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

// LongWindowSet::export_autocorr: rows [copied - min(copied, W), copied), as export_trend
int LongWindowSet::export_autocorr(uint32_t span, const float* scale, uint32_t L, int64_t* dst, void* stream_ptr) {
  if (bad_autocorr(span, scale, L, dst)) return hipErrorInvalidValue;
  for (const auto& r : rings_)
    if (r.ring->width() > kMaxAutocorrStride) return hipErrorInvalidValue;
  if (ingest_pending_) return hipErrorNotReady;  // staged rows no kernel has written yet: refresh() first
  auto stream = static_cast<hipStream_t>(stream_ptr);
  DeviceScope scope(device_);
  const hipError_t e = zero(dst, nseries_, L, stream);
  if (e != hipSuccess) return e;
  for (const auto& r : rings_) {
    const uint32_t wd = r.ring->width();
    const int err = run(r.dev.get<float>(), wd, wd, window_, r.copied, std::min<uint64_t>(r.copied, window_), span,
                        scale + r.first_series, L, dst + size_t(r.first_series) * (L + 1) * 4, stream);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace rocmdash
