// Exact integer lead/lag sums of pairs of series of a time-major device ring (see window_xcorr.h).
#include "window_xcorr.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "device_scope.h"
#include "device_window.h"
#include "long_window.h"
#include "window_lag_dev.h"

namespace rocmdash {
namespace {

using namespace lag;

constexpr int kNT = int(kThreads);  // 220 VGPRs: 2 waves per SIMD, two workgroups share a CU
constexpr uint32_t kR = 2 * kXcorrGroupPairs;  // LDS rows, and directed items, of a workgroup
constexpr uint32_t kLB = kXcorrLagBlock;
static_assert(kLB % kKT == 0 && kR * (kLB / kKT) == kNT && kR == kRows, "one item per thread, one loader column per row");

struct XcorrArgs {
  const float* base;        // the ring's first float
  const float* scale;       // [cols]
  unsigned long long* dst;  // [K][2L + 1][6], zeroed in stream order
  uint64_t first;           // the span's oldest row: head - N
  uint32_t stride, mask, N, L, chunks, share, count;  // mask: depth - 1; share: chunks of a workgroup; count: pairs
  uint8_t col[2 * kMaxXcorrPairs];                    // row 2i: pair i's a, row 2i + 1: its b
  uint8_t slot[kMaxXcorrPairs];                       // pair i's k of dst
};

struct Sums {  // one thread's: n, Sx and Sy of a whole span fit 32 bits
  uint32_t n[kKT] = {}, sx[kKT] = {}, sy[kKT] = {};
  uint64_t sxy[kKT] = {}, sxx[kKT] = {}, syy[kKT] = {};
};

// One thread's chunk: lags k0 .. k0 + 7 of x[t] against y[t + k] over rows [0, tend), tend a
// multiple of 16; wy points at y's word k0. Words past the span are invalid with q = 0, so no
// row needs a bound.
template <Walk kW>
__device__ inline void tile(const uint16_t* wx, const uint16_t* wy, uint32_t tend, Sums& s) {
  const uint4* const xr = reinterpret_cast<const uint4*>(wx);
  const uint4* const yr = reinterpret_cast<const uint4*>(wy);
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
      if (kW == kXY || kW == kXYandY) s.sxy[j] += p1[j];
      if (kW == kXYandY) s.sy[j] += p2[j];
      if (kW == kNXandXX) {
        s.n[j] += p1[j] & 0xffu;
        s.sx[j] += p1[j] >> 8;
        s.sxx[j] += p2[j];
      }
      if (kW == kYY) s.syy[j] += p1[j];
    }
  }
}

// sums of q and of q^2 over words [0, e) of a row: its block prefixes and the first e % 8 words of the block
__device__ inline void prefix(const uint16_t* ws, const uint32_t* pbs, const uint64_t* pbs2, uint32_t e, uint32_t& r,
                              uint64_t& r2) {
  uint32_t q[8];
  unpack_q(reinterpret_cast<const uint4*>(ws)[e >> 3], q);
  r = pbs[e >> 3];
  uint32_t part = 0;
#pragma unroll
  for (uint32_t i = 0; i < 7; ++i) {
    const uint32_t qi = i < (e & 7u) ? q[i] : 0u;
    r += qi;
    part = mad24(qi, qi, part);  // 7 x 4095^2 < 2^32
  }
  r2 = pbs2[e >> 3] + part;
}

// grid (shares of chunks, groups of 4 pairs, blocks of kLB lags). Per chunk: (1) the rows
// [t0, t0 + len) of the span - the chunk and the halo this block's lags reach - are read 8 lanes
// per ring row, lane c the column of LDS row c (two arbitrary columns per pair, all of one ring
// row: the same cache lines), rows in order, 4 loads in flight per lane, quantised and stored as
// words [row][time]; rows past the span are stored as invalid; a NaN marks its LDS row. (2) a
// wave per LDS row sums q and q^2 per block of 8 words and scans the sums into pb (32 bits) and
// pb2 (64 bits): the exclusive prefixes at every 8th word. (3) every thread runs its (item, 8
// lags): an item with both rows clean takes n, Sx, Sy, Sxx and Syy from the prefixes - all rows
// of the chunk are valid, so vy[t + k] is 1 exactly while t + k is in the span - and Sxy from the
// loop; an item with a marked row takes all six from the loop. The sums of a workgroup's chunks
// stay in registers; at the end each non-zero one is added to dst with one vector atomic.
__global__ __launch_bounds__(kNT) void xcorr_ring_kernel(const XcorrArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t w[kR * kPitch];
  __shared__ uint64_t pb2[kR * kPBPitch];
  __shared__ uint32_t pb[kR * kPBPitch];
  __shared__ uint32_t marked[kR];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t gs = xcorr_group_rows(a.count, blockIdx.y);  // this group's LDS rows: two per pair
  const uint32_t klo = blockIdx.z * kLB, khi = xcorr_block_hi(a.L, blockIdx.z);
  const uint32_t tiles = xcorr_block_tiles(a.L, blockIdx.z);
  const uint32_t len = xcorr_load_rows(khi);  // <= kPitch
  const uint32_t nb = len >> 3;
  const uint32_t c1 = min((blockIdx.x + 1) * a.share, a.chunks);
  uint32_t r, tile_i;  // the directed item: x = row r, y = row r ^ 1
  const bool mine = xcorr_thread(tid, gs, tiles, &r, &tile_i);
  const uint32_t k0 = klo + tile_i * kKT;
  const uint16_t* const wx = w + r * kPitch;
  const uint16_t* const wy = w + (r ^ 1u) * kPitch;
  const uint32_t* const pbx = pb + r * kPBPitch;
  const uint32_t* const pby = pb + (r ^ 1u) * kPBPitch;
  const uint64_t* const pbx2 = pb2 + r * kPBPitch;
  const uint64_t* const pby2 = pb2 + (r ^ 1u) * kPBPitch;
  const uint32_t lr = tid & 7u;  // the loader's LDS row: kNT is a multiple of 8
  const uint32_t lcol = lr < gs ? a.col[blockIdx.y * kR + lr] : 0u;
  const float sc = lr < gs ? a.scale[lcol] : 0.f;

  Sums s;
  for (uint32_t c = blockIdx.x * a.share; c < c1; ++c) {
    const uint32_t t0 = c * kT, left = a.N - t0, rows = min(kT, left);
    __syncthreads();  // the last chunk's readers are done
    if (tid < kR) marked[tid] = 0u;
    __syncthreads();
#pragma unroll 1
    for (uint32_t e0 = tid; e0 < len * 8u; e0 += kNT * 4) {
      float x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t p = (e0 + uint32_t(u) * kNT) >> 3;
        const bool in = p < len && p < left && lr < gs;  // a row of the span: slot < depth, column < cols
        const uint64_t slot = (a.first + t0 + p) & a.mask;
        x[u] = in ? a.base[slot * a.stride + lcol] : __builtin_nanf("");
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t p = (e0 + uint32_t(u) * kNT) >> 3;
        if (p >= len || lr >= gs) continue;
        uint32_t word = kInvalid;
        if (!isnan(x[u]))
          word = uint32_t(fminf(fmaxf(rintf(x[u] * sc), 0.f), float(kAutocorrQMax)));
        else if (p < left)
          marked[lr] = 1u;  // the same value from every writer
        w[lr * kPitch + p] = uint16_t(word);
      }
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t row_i = wave; row_i < gs; row_i += kNT / 64) {
      const uint4* const row = reinterpret_cast<const uint4*>(w + row_i * kPitch);
      uint32_t bs[kPerLane], bs2[kPerLane], tot = 0, tot2 = 0;  // 5 blocks of q^2: 40 x 4095^2 < 2^32
#pragma unroll
      for (uint32_t u = 0; u < kPerLane; ++u) {
        const uint32_t j = lane * kPerLane + u;
        bs[u] = bs2[u] = 0;
        if (j < nb) {
          uint32_t q[8];
          unpack_q(row[j], q);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            bs[u] += q[i];
            bs2[u] = mad24(q[i], q[i], bs2[u]);
          }
        }
        tot += bs[u];
        tot2 += bs2[u];
      }
      uint32_t inc = tot;
      unsigned long long inc2 = tot2;
#pragma unroll
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        const unsigned long long o2 = __shfl_up(inc2, d);
        if (lane >= d) {
          inc += o;
          inc2 += o2;
        }
      }
      uint32_t run = inc - tot;
      uint64_t run2 = inc2 - tot2;
#pragma unroll
      for (uint32_t u = 0; u < kPerLane; ++u) {
        const uint32_t j = lane * kPerLane + u;
        if (j <= nb) {
          pb[row_i * kPBPitch + j] = run;
          pb2[row_i * kPBPitch + j] = run2;
        }
        run += bs[u];
        run2 += bs2[u];
      }
    }
    __syncthreads();
    if (!mine) continue;  // barriers are at the loop's head: every thread reaches them
    const uint32_t tend = (rows + 15) & ~15u;
    if (marked[r] | marked[r ^ 1u]) {
      tile<kXYandY>(wx, wy + k0, tend, s);
      tile<kNXandXX>(wx, wy + k0, tend, s);
      tile<kYY>(wx, wy + k0, tend, s);
    } else {
      tile<kXY>(wx, wy + k0, tend, s);
      // Sy_k and Syy_k = sums over y's words [k, tend + k): the words from the span's end on are 0,
      // and both ends are j words into a block
      uint32_t ql[8], qh[8];
      unpack_q(reinterpret_cast<const uint4*>(wy + k0)[0], ql);
      unpack_q(reinterpret_cast<const uint4*>(wy + k0)[tend >> 3], qh);
      uint32_t syk = pby[(tend + k0) >> 3] - pby[k0 >> 3];
      uint64_t syyk = pby2[(tend + k0) >> 3] - pby2[k0 >> 3];
      const bool inner = left >= rows + k0 + kKT;  // every t + k is in the span: n_k = rows
      const uint32_t whole = pbx[(rows + 7) >> 3];  // rows % 8 != 0 only in the span's last chunk, 0 from there on
      const uint64_t whole2 = pbx2[(rows + 7) >> 3];
#pragma unroll
      for (uint32_t j = 0; j < kKT; ++j) {
        const uint32_t k = k0 + j;
        const uint32_t nk = k < left ? min(rows, left - k) : 0u;  // rows t of the chunk with t + k in the span
        uint32_t px = whole;
        uint64_t px2 = whole2;
        if (!inner) prefix(wx, pbx, pbx2, nk, px, px2);
        s.n[j] += nk;
        s.sx[j] += px;
        s.sxx[j] += px2;
        s.sy[j] += syk;
        s.syy[j] += syyk;
        syk += qh[j] - ql[j];
        syyk += uint64_t(mad24(qh[j], qh[j], 0u)) - uint64_t(mad24(ql[j], ql[j], 0u));
      }
    }
  }
  if (!mine) return;
  const uint32_t slot = a.slot[blockIdx.y * kXcorrGroupPairs + (r >> 1)];
  const bool swap = (r & 1u) != 0;  // (b, a) at lag k is (a, b) at lag -k with the x and the y words swapped
#pragma unroll
  for (uint32_t j = 0; j < kKT; ++j) {
    const int32_t idx = xcorr_index(a.L, r, k0 + j);
    if (idx < 0) continue;
    unsigned long long* const d = a.dst + (size_t(slot) * (2 * a.L + 1) + uint32_t(idx)) * kXcorrWords;
    if (s.n[j]) atomicAdd(d + 0, static_cast<unsigned long long>(s.n[j]));
    if (s.sx[j]) atomicAdd(d + (swap ? 2 : 1), static_cast<unsigned long long>(s.sx[j]));
    if (s.sy[j]) atomicAdd(d + (swap ? 1 : 2), static_cast<unsigned long long>(s.sy[j]));
    if (s.sxy[j]) atomicAdd(d + 3, static_cast<unsigned long long>(s.sxy[j]));
    if (s.sxx[j]) atomicAdd(d + (swap ? 5 : 4), static_cast<unsigned long long>(s.sxx[j]));
    if (s.syy[j]) atomicAdd(d + (swap ? 4 : 5), static_cast<unsigned long long>(s.syy[j]));
  }
}

// the pairs p of one ring of `depth` rows over its span [head - min(n, span), head) onto dst (already
// zeroed); share 0: xcorr_share's rule, else the chunks of a workgroup, checked by the caller
inline int run(const XcorrRingPairs& p, const float* base, uint32_t stride, uint64_t depth, uint64_t head, uint64_t n,
               uint32_t span, const float* scale, uint32_t L, int64_t* dst, hipStream_t stream, uint32_t share = 0) {
  const uint32_t N = uint32_t(std::min<uint64_t>(n, span));
  if (head == 0 || N == 0 || p.count == 0) return hipSuccess;  // the zeroes stand
  XcorrArgs a{};
  a.base = base;
  a.scale = scale;
  a.dst = reinterpret_cast<unsigned long long*>(dst);
  a.first = head - N;
  a.stride = stride;
  a.mask = uint32_t(depth - 1);
  a.N = N;
  a.L = L;
  a.chunks = (N + kT - 1) / kT;
  a.count = p.count;
  for (uint32_t i = 0; i < p.count; ++i) {
    a.col[2 * i] = p.a[i];
    a.col[2 * i + 1] = p.b[i];
    a.slot[i] = p.slot[i];
  }
  const uint32_t groups = xcorr_pair_groups(p.count), blocks = xcorr_lag_blocks(L);
  a.share = share ? share : xcorr_share(a.chunks, groups * blocks);
  hipLaunchKernelGGL(xcorr_ring_kernel, dim3(xcorr_share_groups(a.chunks, a.share), groups, blocks), dim3(kNT), 0, stream, a);
  return hipGetLastError();
}

inline hipError_t zero(int64_t* dst, uint32_t K, uint32_t L, hipStream_t stream) {
  return hipMemsetAsync(dst, 0, size_t(K) * (2 * L + 1) * kXcorrWords * sizeof(int64_t), stream);
}

}  // namespace

int launch_xcorr_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                      uint32_t span, const float* scale, const uint32_t* pairs, uint32_t K, uint32_t L, int64_t* dst,
                      void* stream_ptr, uint32_t share) {
  if (bad_xcorr(span, scale, pairs, K, L, dst) || base == nullptr || !pow2(depth) || n > depth || n > head || stride < 1 ||
      stride > kMaxAutocorrStride || cols < 1 || cols > stride)
    return hipErrorInvalidValue;
  if (share > std::max(1u, (std::min(n, span) + kT - 1) / kT)) return hipErrorInvalidValue;  // 0: the rule
  const XcorrRingSpan ring{0, cols};
  XcorrPlan plan;
  if (!xcorr_plan_pairs(pairs, K, &ring, 1, &plan)) return hipErrorInvalidValue;
  auto stream = static_cast<hipStream_t>(stream_ptr);
  const hipError_t e = zero(dst, K, L, stream);
  if (e != hipSuccess) return e;
  return run(plan.rings[0], base, stride, depth, head, n, span, scale, L, dst, stream, share);
}

// DeviceWindowSet::export_xcorr lives here with its kernel (device_window.h declares it); the
// window is export_autocorr's. A ring without a pair is not streamed.
int DeviceWindowSet::export_xcorr(const uint32_t* pairs, uint32_t K, uint32_t span, const float* scale, uint32_t L,
                                  int64_t* dst, void* stream_ptr) const {
  if (bad_xcorr(span, scale, pairs, K, L, dst)) return hipErrorInvalidValue;
  std::vector<XcorrRingSpan> spans;
  for (const auto& r : rings_) spans.push_back(XcorrRingSpan{r.first_series, r.ring->width()});
  XcorrPlan plan;
  if (!xcorr_plan_pairs(pairs, K, spans.data(), uint32_t(spans.size()), &plan)) return hipErrorInvalidValue;
  auto stream = static_cast<hipStream_t>(stream_ptr);
  DeviceScope scope(device_);
  const hipError_t e = zero(dst, K, L, stream);
  if (e != hipSuccess) return e;
  for (uint32_t i = 0; i < plan.nrings; ++i) {
    const auto& r = rings_[plan.rings[i].ring];
    const int err = run(plan.rings[i], r.dev, r.ring->width(), dev_rows(), r.state_valid ? r.last_head : 0,
                        r.state_valid ? r.last_n : 0, span, scale + r.first_series, L, dst, stream);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

// LongWindowSet::export_xcorr: rows [copied - min(copied, W), copied), as export_autocorr
int LongWindowSet::export_xcorr(const uint32_t* pairs, uint32_t K, uint32_t span, const float* scale, uint32_t L, int64_t* dst,
                                void* stream_ptr) {
  if (bad_xcorr(span, scale, pairs, K, L, dst)) return hipErrorInvalidValue;
  std::vector<XcorrRingSpan> spans;
  for (const auto& r : rings_) spans.push_back(XcorrRingSpan{r.first_series, r.ring->width()});
  XcorrPlan plan;
  if (!xcorr_plan_pairs(pairs, K, spans.data(), uint32_t(spans.size()), &plan)) return hipErrorInvalidValue;
  if (ingest_pending_) return hipErrorNotReady;  // staged rows no kernel has written yet: refresh() first
  auto stream = static_cast<hipStream_t>(stream_ptr);
  DeviceScope scope(device_);
  const hipError_t e = zero(dst, K, L, stream);
  if (e != hipSuccess) return e;
  for (uint32_t i = 0; i < plan.nrings; ++i) {
    const auto& r = rings_[plan.rings[i].ring];
    const int err = run(plan.rings[i], r.dev.get<float>(), r.ring->width(), window_, r.copied,
                        std::min<uint64_t>(r.copied, window_), span, scale + r.first_series, L, dst, stream);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace rocmdash
