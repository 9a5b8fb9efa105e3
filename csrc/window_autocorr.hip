// Exact integer lag sums of every series of a time-major device ring (see window_autocorr.h).
#include "window_autocorr.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_window.h"
#include "long_window.h"

namespace rocmdash {
namespace {

constexpr int kNT = 256;                 // 4 waves; 184 VGPRs: 2 waves per SIMD, two workgroups share a CU
constexpr uint32_t kT = kAutocorrChunk;  // rows of a chunk
constexpr uint32_t kKT = 8;              // consecutive lags a thread owns: one 16-byte LDS read
constexpr uint32_t kG = 8;               // series of a workgroup
constexpr uint32_t kLB = 256;             // lags of a workgroup: every thread owns one (series, 8 lags)
constexpr uint32_t kPitch = kT + kMaxAutocorrLags + 16;  // words of a series: chunk, halo, the last read's reach
constexpr uint32_t kBlocks = kPitch / 8;                 // 8-word blocks of a series
constexpr uint32_t kPBPitch = kBlocks + 2;
constexpr uint32_t kPerLane = (kBlocks + 63) / 64;  // blocks a lane sums in the prefix scan
constexpr uint32_t kFold = 128;                     // rows an int32 partial takes: 128 x 4095^2 < 2^31
constexpr uint32_t kInvalid = 0x8000u;              // bit 15 of a word: no sample (NaN, or past the span)
constexpr uint32_t kTargetGroups = 1024;            // workgroups of a launch: two rounds of 2 per CU
static_assert(kPitch % 8 == 0 && (kPitch * 2) % 16 == 0 && kLB % kKT == 0 && kT % 16 == 0, "16-byte LDS reads");
static_assert(kG * (kLB / kKT) == kNT, "one item per thread");

struct AutocorrArgs {
  const float* base;        // the ring's first float
  const float* scale;       // [cols]
  unsigned long long* dst;  // [cols][L + 1][4], zeroed in stream order
  uint64_t first;           // the span's oldest row: head - N
  uint32_t stride, cols, mask, N, L, chunks, share;  // mask: depth - 1; share: chunks of a workgroup
};

__device__ inline uint32_t lo12(uint32_t w) { return w & 0xfffu; }
__device__ inline uint32_t hi12(uint32_t w) { return (w >> 16) & 0xfffu; }

// a x b + c, a and b below 2^24: one full-rate instruction, and stated as one. Written as
// a * b + c or with __umul24, ROCm 7.2.0 (AMD clang 22.0.0git, roc-7.2.0) combines the chains of
// products of 12-bit fields into v_dot4_u32_u8, which keeps 8 bits of each factor: the sums of
// lags 1 - 3 and 5 - 7 of every 8 are short for q above 255. Plain C++ can return once a
// compiler no longer does that; tests/test_gpu_window_autocorr.py would show it.
__device__ inline uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// the q of 8 consecutive words
__device__ inline void unpack_q(const uint4 p, uint32_t (&q)[8]) {
  const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    q[2 * i] = lo12(w[i]);
    q[2 * i + 1] = hi12(w[i]);
  }
}

// their validity: 1 for a sample, 0 for none
__device__ inline void unpack_v(const uint4 p, uint32_t (&v)[8]) {
  const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = (~w[i] >> 15) & 1u;
    v[2 * i + 1] = ~w[i] >> 31;
  }
}

// What a walk over the chunk sums. kXY: Sxy alone - all a clean series needs from the loop.
// kXYandY: Sxy and Sy, kNandX: n and Sx - the two walks of a series with an invalid sample, two
// so that either stays within the registers of the first.
enum Walk { kXY, kXYandY, kNandX };

// the x side of 8 rows: x1 multiplies into p1, x2 (kXYandY only) into p2
template <Walk kW>
__device__ inline void unpack_x(const uint4 p, uint32_t (&x1)[8], uint32_t (&x2)[8]) {
  unpack_q(p, x1);
  if (kW == kXYandY) unpack_v(p, x2);
  if (kW == kNandX) {  // n in bits 0-7 (at most 128 per fold), Sx in bits 8-31 (at most 128 x 4095)
    unpack_v(p, x2);
#pragma unroll
    for (int i = 0; i < 8; ++i) x1[i] = x2[i] | (x1[i] << 8);
  }
}

template <Walk kW>
__device__ inline void unpack_y(const uint4 p, uint32_t (&y)[8]) {
  if (kW == kNandX)
    unpack_v(p, y);
  else
    unpack_q(p, y);
}

// 8 rows x 8 lags: x = rows t .. t + 7, (ya, yb) = rows t + k0 .. t + k0 + 15; every factor is below 2^24
template <Walk kW>
__device__ inline void mac(const uint32_t (&x1)[8], const uint32_t (&x2)[8], const uint32_t (&ya)[8], const uint32_t (&yb)[8],
                           uint32_t (&p1)[kKT], uint32_t (&p2)[kKT]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = 0; j < int(kKT); ++j) {
      const int e = i + j;
      const uint32_t y = e < 8 ? ya[e & 7] : yb[e & 7];
      p1[j] = mad24(x1[i], y, p1[j]);
      if (kW == kXYandY) p2[j] = mad24(x2[i], y, p2[j]);
    }
  }
}

// One thread's chunk: lags k0 .. k0 + 7 of the series at ws over rows [0, tend), tend a multiple
// of 16. Words past the span are invalid with q = 0, so no row needs a bound. kXY and kXYandY add
// to (s1, s2) = (Sxy, Sy), kNandX to (n, Sx).
template <Walk kW>
__device__ inline void tile(const uint16_t* ws, uint32_t k0, uint32_t tend, uint64_t (&s1)[kKT], uint64_t (&s2)[kKT]) {
  const uint4* const xr = reinterpret_cast<const uint4*>(ws);
  const uint4* const yr = reinterpret_cast<const uint4*>(ws + k0);
  uint32_t ya[8], yb[8], x1[8], x2[8];
  unpack_y<kW>(yr[0], ya);
#pragma unroll 1
  for (uint32_t t = 0; t < tend; t += kFold) {
    uint32_t p1[kKT] = {}, p2[kKT] = {};
    const uint32_t ue = min(t + kFold, tend) >> 3;
#pragma unroll 1
    for (uint32_t u = t >> 3; u < ue; u += 2) {  // the window of 16 y slides by 8: (a, b) then (b, a)
      unpack_x<kW>(xr[u], x1, x2);
      unpack_y<kW>(yr[u + 1], yb);
      mac<kW>(x1, x2, ya, yb, p1, p2);
      unpack_x<kW>(xr[u + 1], x1, x2);
      unpack_y<kW>(yr[u + 2], ya);
      mac<kW>(x1, x2, yb, ya, p1, p2);
    }
#pragma unroll
    for (int j = 0; j < int(kKT); ++j) {
      if (kW == kNandX) {
        s1[j] += p1[j] & 0xffu;
        s2[j] += p1[j] >> 8;
      } else {
        s1[j] += p1[j];
        if (kW == kXYandY) s2[j] += p2[j];
      }
    }
  }
}

// sum of q over words [0, e) of a series: its block prefix and the first e % 8 words of the block
__device__ inline uint32_t prefix(const uint16_t* ws, const uint32_t* pbs, uint32_t e) {
  uint32_t q[8];
  unpack_q(reinterpret_cast<const uint4*>(ws)[e >> 3], q);
  uint32_t r = pbs[e >> 3];
#pragma unroll
  for (uint32_t i = 0; i < 7; ++i) r += i < (e & 7u) ? q[i] : 0u;
  return r;
}

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

inline bool pow2(uint64_t x) { return x != 0 && (x & (x - 1)) == 0; }

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
