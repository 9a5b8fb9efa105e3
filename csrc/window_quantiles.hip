// Exact percentiles of every trend column of the windows in the time-major device rings (see
// window_quantiles.h).
#include "window_quantiles.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "device_scope.h"
#include "device_window.h"
#include "long_window.h"
#include "long_window_dev.h"
#include "window_stats_rules.h"
#include "window_trend.h"

namespace rocmdash {
namespace {

constexpr int kUnroll = 8;             // loads a lane has in flight before it uses any of them
constexpr uint32_t kRanks = 6;         // lo0, hi0, lo1, hi1, lo2, hi2
constexpr int kSelectNT = 1024;        // the radix select: one workgroup of 16 waves
constexpr uint32_t kSelectSeries = 16; // ... owns up to this many series of a slot
// one series' histograms [rank][256], + 4 words so that the series do not share a bank
constexpr uint32_t kHistPitch = kRanks * 256 + 4;
// the LDS sort: keys a workgroup of 1 / 4 / 16 waves holds (a wave's is the trend's
// kWaveSlotFloats); a ring with more keys per slot is cut into groups of series
constexpr uint32_t kSortKeys1 = 2048, kSortKeys4 = 8192, kSortKeys16 = 16384;
static_assert(kQuantileSortMaxRows <= kSortKeys16, "one series' column fits the largest sort");

struct QuantRing {
  const float* base;  // device ring: row r at base + (r & mask) * stride
  float* dst;         // the ring's first series' [P + 1][4]
  uint64_t head;
  uint32_t stride, cols, mask, n;
};

struct QuantArgs {
  QuantRing r[kTrendRingsPerLaunch];  // blockIdx.y
  double qfrac[3];                    // double(float(pct)) / 100
  uint32_t log2c, P;
  uint32_t gs;  // series per workgroup: blockIdx.z owns series [z * gs, z * gs + gs) of its ring
};

// The rows of slot j, as trend_slot_rows of window_trend.hip (the one statement of them is
// rocmdash.ops.window_trend.trend_geometry): [lo, hi), lo == hi when the slot is empty. Uniform.
__device__ __forceinline__ void quant_slot_rows(uint64_t head, uint32_t n, uint32_t log2c, uint32_t P, uint32_t j,
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

// The stream is trend_slot's: the slot's block of F = rows x stride contiguous floats is cut
// into pieces of L floats - L the largest multiple of the stride a wave holds, so lane l stays
// on series l % stride - and wave w takes the pieces w, w + NW, ...: coalesced 4-byte loads,
// kUnroll of them in flight per lane. f(x, piece) runs on every lane of the wave, in
// convergent code, with NaN for what a lane does not read.
template <int NW, class Fn>
__device__ __forceinline__ void quant_stream(const float* p, uint32_t F, uint32_t L, uint32_t lane, uint32_t wave, Fn&& f) {
  for (uint32_t k0 = wave; uint64_t(k0) * L < F; k0 += NW * kUnroll) {
    float v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint64_t i = uint64_t(k0 + uint32_t(u) * NW) * L + lane;
      v[u] = (lane < L && i < F) ? p[i] : __builtin_nanf("");
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) f(v[u], k0 + uint32_t(u) * NW);
  }
}

// percentile_between, but for one case: where the percentile IS an order statistic (frac == 0
// or x0 == x1) and one of the two is infinite, the arithmetic would make NaN of it (inf - inf,
// inf x 0) - the order statistic is returned as it is. Finite values take the arithmetic alone.
__device__ __forceinline__ float quant_between(float x0, float x1, float frac) {
  if ((frac == 0.f || x0 == x1) && !(isfinite(x0) && isfinite(x1))) return x0;
  return percentile_between(x0, x1, frac);
}

// {p_a, p_b, p_c, count} of one (series, slot) from its six order statistics (keys)
__device__ __forceinline__ void quant_store(const QuantRing& R, uint32_t P, uint32_t j, uint32_t series, uint32_t nv,
                                            const uint32_t (&k)[kRanks], const float (&frac)[3]) {
  const float nan = __builtin_nanf("");
  float4 o{nan, nan, nan, 0.f};
  if (nv)
    o = float4{quant_between(kfloat(k[0]), kfloat(k[1]), frac[0]), quant_between(kfloat(k[2]), kfloat(k[3]), frac[1]),
               quant_between(kfloat(k[4]), kfloat(k[5]), frac[2]), float(nv)};
  reinterpret_cast<float4*>(R.dst)[size_t(series) * (P + 1) + j] = o;
}

__device__ __forceinline__ void quant_store_empty(const QuantRing& R, uint32_t P, uint32_t j, uint32_t series) {
  const float nan = __builtin_nanf("");
  reinterpret_cast<float4*>(R.dst)[size_t(series) * (P + 1) + j] = float4{nan, nan, nan, 0.f};
}

// ---- small slots: sort in LDS ---------------------------------------------------------
// grid (slots, rings, groups of series). The slot's keys go to LDS as [series][c], NaNs and
// the rows a partial slot lacks as 0xFFFFFFFF, which no valid sample keys to; one spare word
// per segment keeps the lanes of a load (consecutive series, the same row) off one bank. A
// bitonic network over the whole array sorts every segment at once: up to the last merge
// neighbouring runs alternate in direction, the last one (k = c) is ascending everywhere.
template <int NW, uint32_t K>
__global__ __launch_bounds__(NW * 64) void quant_sort_kernel(const QuantArgs a) {
  constexpr uint32_t NT = NW * 64;
  __shared__ uint32_t keys[K + kMaxTrendStride];
  __shared__ uint32_t cnt[kMaxTrendStride];
  const QuantRing& R = a.r[blockIdx.y];
  const uint32_t j = blockIdx.x, g0 = blockIdx.z * a.gs, tid = threadIdx.x;
  if (g0 >= R.cols) return;  // uniform: the whole workgroup, before any barrier
  const uint32_t gs = min(a.gs, R.cols - g0);
  const uint32_t log2c = a.log2c, c = 1u << log2c, N = gs << log2c;  // N <= K
  uint64_t rlo, rhi;
  quant_slot_rows(R.head, R.n, log2c, a.P, j, rlo, rhi);
  const uint32_t rows = uint32_t(rhi - rlo);
  if (rows == 0) {  // uniform
    if (tid < gs) quant_store_empty(R, a.P, j, g0 + tid);
    return;
  }
  auto phys = [&](uint32_t i) { return i + (i >> log2c); };
  for (uint32_t i = tid; i < N; i += NT) keys[phys(i)] = 0xFFFFFFFFu;
  if (tid < gs) cnt[tid] = 0u;
  __syncthreads();

  {
    const uint32_t stride = R.stride, per = 64u / stride, L = per * stride;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = NW > 1 ? uint32_t(__builtin_amdgcn_readfirstlane(int(tid >> 6))) : 0u;
    const uint32_t s = lane % stride - g0, r0 = lane / stride;  // s >= gs: not this workgroup's
    const float* p = R.base + size_t(rlo & R.mask) * stride;
    uint32_t valid = 0;
    quant_stream<NW>(p, rows * stride, L, lane, wave, [&](float x, uint32_t piece) {
      if (isnan(x) || s >= gs) return;
      keys[phys((s << log2c) + piece * per + r0)] = fkey(x);  // the row within the slot: < rows
      ++valid;
    });
    if (valid) atomicAdd(&cnt[s], valid);
  }
  __syncthreads();

  for (uint32_t k = 2; k <= c; k <<= 1)
    for (uint32_t d = k >> 1; d > 0; d >>= 1) {
      for (uint32_t t = tid; t < N / 2; t += NT) {
        const uint32_t i = ((t & ~(d - 1)) << 1) | (t & (d - 1)), i2 = i | d;  // d < c: one segment
        const bool asc = k == c || !(i & k);
        const uint32_t x = keys[phys(i)], y = keys[phys(i2)];
        if ((x > y) == asc && x != y) {
          keys[phys(i)] = y;
          keys[phys(i2)] = x;
        }
      }
      __syncthreads();
    }

  if (tid < gs) {
    const uint32_t nv = cnt[tid];
    uint32_t idx[8], k[kRanks];
    float frac[3];
    wanted_positions(nv, a.qfrac, idx, frac);
#pragma unroll
    for (uint32_t r = 0; r < kRanks; ++r) k[r] = keys[phys((tid << log2c) + idx[2 + r])];
    quant_store(R, a.P, j, g0 + tid, nv, k, frac);
  }
}

// ---- large slots: MSD radix select over LDS histograms ---------------------------------
// grid (slots, rings, groups of kSelectSeries series). Pass A streams the slot for every
// series' min / max key and count; the keys of a series differ only below bit hb = the
// highest bit in which min and max differ, so its six ranks are found in ceil(hb / 8) digit
// passes, each streaming the slot again (from L2 / MALL where it fits) and counting, per
// rank, the digit [lo, hi) of the keys that match the rank's prefix above hi. Ranks whose
// prefixes have not diverged share one histogram (the lowest such rank's). Where every lane
// of a wave holds the key bits of its series' first lane, that lane adds for all of them.
// A bin counts up to 65536 equal samples: 32 bits.
__global__ __launch_bounds__(kSelectNT) void quant_select_kernel(const QuantArgs a) {
  constexpr int NW = kSelectNT / 64;
  __shared__ uint32_t hist[kSelectSeries * kHistPitch];
  __shared__ uint32_t smn[kSelectSeries], smx[kSelectSeries], scnt[kSelectSeries], shb[kSelectSeries];
  __shared__ uint32_t spre[2][kSelectSeries][kRanks], srank[2][kSelectSeries][kRanks];
  __shared__ uint32_t passes;
  const QuantRing& R = a.r[blockIdx.y];
  const uint32_t j = blockIdx.x, g0 = blockIdx.z * kSelectSeries, tid = threadIdx.x;
  if (g0 >= R.cols) return;  // uniform: the whole workgroup, before any barrier
  const uint32_t gs = min(kSelectSeries, R.cols - g0);
  uint64_t rlo, rhi;
  quant_slot_rows(R.head, R.n, a.log2c, a.P, j, rlo, rhi);
  const uint32_t rows = uint32_t(rhi - rlo);
  if (rows == 0) {  // uniform
    if (tid < gs) quant_store_empty(R, a.P, j, g0 + tid);
    return;
  }
  const uint32_t stride = R.stride, per = 64u / stride, L = per * stride;
  const uint32_t F = rows * stride;  // <= 65536 x 64 floats
  const uint32_t lane = tid & 63u, wave = uint32_t(__builtin_amdgcn_readfirstlane(int(tid >> 6)));
  const uint32_t s = lane % stride - g0, r0 = lane / stride;
  const bool mine = lane < L && s < gs;  // this lane reads a series of this workgroup
  const float* p = R.base + size_t(rlo & R.mask) * stride;

  if (tid < gs) {
    smn[tid] = 0xFFFFFFFFu;
    smx[tid] = 0u;
    scnt[tid] = 0u;
  }
  if (tid == 0) passes = 0u;
  __syncthreads();

  {  // pass A
    uint32_t mn = 0xFFFFFFFFu, mx = 0u, cnt = 0u;
    quant_stream<NW>(p, F, L, lane, wave, [&](float x, uint32_t) {
      if (isnan(x) || !mine) return;
      const uint32_t k = fkey(x);
      mn = min(mn, k);
      mx = max(mx, k);
      ++cnt;
    });
    if (cnt) {
      atomicMin(&smn[s], mn);
      atomicMax(&smx[s], mx);
      atomicAdd(&scnt[s], cnt);
    }
  }
  __syncthreads();

  if (tid < gs) {
    const uint32_t nv = scnt[tid], mn = smn[tid], diff = nv ? mn ^ smx[tid] : 0u;
    const uint32_t hb = diff ? 32u - uint32_t(__builtin_clz(diff)) : 0u;
    uint32_t idx[8];
    float frac[3];
    wanted_positions(nv, a.qfrac, idx, frac);
    const uint32_t top = uint32_t((uint64_t(mn) >> hb) << hb);  // the bits every key of the series shares
#pragma unroll
    for (uint32_t r = 0; r < kRanks; ++r) {
      spre[0][tid][r] = top;
      srank[0][tid][r] = idx[2 + r];
    }
    shb[tid] = hb;
    atomicMax(&passes, (hb + 7u) / 8u);
  }
  __syncthreads();
  const uint32_t np = passes;
  const uint32_t hb = mine ? shb[s] : 0u;

  for (uint32_t ps = 0; ps < np; ++ps) {
    const uint32_t cur = ps & 1u, nxt = cur ^ 1u;
    for (uint32_t i = tid; i < gs * kHistPitch; i += kSelectNT) hist[i] = 0u;
    __syncthreads();  // (the prefixes of this pass were written before the last barrier too)

    {
      const bool part = mine && hb > 8u * ps;  // the series still has a digit to find
      const uint32_t hi = part ? hb - 8u * ps : 32u, lo = hi > 8u ? hi - 8u : 0u;
      uint32_t pre[kRanks], own = 0u;  // own: ranks whose prefix no lower rank has
#pragma unroll
      for (uint32_t r = 0; r < kRanks; ++r) {
        pre[r] = part ? spre[cur][s][r] : 0u;
        bool first = part;
#pragma unroll
        for (uint32_t r2 = 0; r2 < r; ++r2) first = first && pre[r2] != pre[r];
        own |= uint32_t(first) << r;
      }
      uint32_t* const h = hist + (part ? s : 0u) * kHistPitch;
      const int leader = int(lane % stride);
      quant_stream<NW>(p, F, L, lane, wave, [&](float x, uint32_t) {
        const bool valid = part && !isnan(x);
        const uint32_t key = fkey(x), w = key >> lo;
        const uint32_t lw = uint32_t(__shfl(int(w), leader));
        const int lvalid = __shfl(int(valid), leader);
        const bool agree = !part || (valid && lvalid && w == lw);
        uint32_t add = valid ? 1u : 0u;
        if (__all(int(agree))) add = (valid && r0 == 0u) ? per : 0u;  // all `per` lanes of the series are valid
        if (!add) return;
#pragma unroll
        for (uint32_t r = 0; r < kRanks; ++r)
          if (((own >> r) & 1u) && (uint64_t(key ^ pre[r]) >> hi) == 0u) atomicAdd(&h[r * 256u + (w & 255u)], add);
      });
    }
    __syncthreads();

    // the digit of every (series, rank): one wave each, 4 bins per lane and a scan over the lanes
    for (uint32_t pair = wave; pair < gs * kRanks; pair += NW) {
      const uint32_t ss = pair / kRanks, r = pair - ss * kRanks;
      const uint32_t pre = spre[cur][ss][r], k = srank[cur][ss][r], shb_s = shb[ss];
      if (shb_s > 8u * ps) {  // uniform
        const uint32_t hi = shb_s - 8u * ps, lo = hi > 8u ? hi - 8u : 0u;
        uint32_t rep = r;
        for (uint32_t r2 = r; r2-- > 0;)
          if (spre[cur][ss][r2] == pre) rep = r2;
        const uint32_t* hb4 = hist + ss * kHistPitch + rep * 256u + lane * 4u;
        const uint32_t b0 = hb4[0], b1 = hb4[1], b2 = hb4[2], b3 = hb4[3];
        const uint32_t t = b0 + b1 + b2 + b3;
        uint32_t inc = t;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t o = uint32_t(__shfl_up(int(inc), off));
          if (lane >= uint32_t(off)) inc += o;
        }
        uint32_t acc = inc - t;
        if (acc <= k && k < inc) {  // one lane: the rank is below the prefix's count
          uint32_t d = 0;
          if (k >= acc + b0) {
            acc += b0;
            d = 1;
            if (k >= acc + b1) {
              acc += b1;
              d = 2;
              if (k >= acc + b2) {
                acc += b2;
                d = 3;
              }
            }
          }
          const uint32_t bin = lane * 4u + d;  // its bits at and above hi - lo are the prefix's
          spre[nxt][ss][r] = (pre & ~(255u << lo)) | (bin << lo);
          srank[nxt][ss][r] = k - acc;
        }
      } else if (lane == 0) {
        spre[nxt][ss][r] = pre;
        srank[nxt][ss][r] = k;
      }
    }
    __syncthreads();
  }

  if (tid < gs) {
    const uint32_t nv = scnt[tid];
    uint32_t idx[8], k[kRanks];
    float frac[3];
    wanted_positions(nv, a.qfrac, idx, frac);
#pragma unroll
    for (uint32_t r = 0; r < kRanks; ++r) k[r] = spre[np & 1u][tid][r];
    quant_store(R, a.P, j, g0 + tid, nv, k, frac);
  }
}

inline uint32_t log2u(uint32_t x) { return 31u - uint32_t(__builtin_clz(x)); }
inline bool bad_columns(uint32_t P) { return P < kMinTrendColumns || P > kMaxTrendColumns || !pow2(P); }
inline bool bad_dst(const float* dst) { return dst == nullptr || (reinterpret_cast<uintptr_t>(dst) & 15u) != 0; }
inline bool bad_pct(float p0, float p1, float p2) {
  for (float p : {p0, p1, p2})
    if (!(p >= 0.f && p <= 100.f)) return true;  // NaN too
  return false;
}
inline void set_pct(QuantArgs& a, float p0, float p1, float p2) {
  a.qfrac[0] = double(p0) / 100.0;
  a.qfrac[1] = double(p1) / 100.0;
  a.qfrac[2] = double(p2) / 100.0;
}

// rings [0, n) of `a0` (every field but gs set, all with rows_per_col = 1 << a.log2c)
void launch(const QuantArgs& a0, uint32_t n, hipStream_t stream) {
  QuantArgs a = a0;
  uint32_t cols = 1;
  for (uint32_t i = 0; i < n; ++i) cols = std::max(cols, a.r[i].cols);
  const uint32_t c = 1u << a.log2c, slots = a.P + 1;
  if (c > kQuantileSortMaxRows) {
    a.gs = kSelectSeries;
    hipLaunchKernelGGL(quant_select_kernel, dim3(slots, n, (cols + kSelectSeries - 1) / kSelectSeries), dim3(kSelectNT), 0,
                       stream, a);
    return;
  }
  const uint32_t want = cols << a.log2c;  // <= 64 x 4096
  const uint32_t K = want <= kSortKeys1 ? kSortKeys1 : want <= kSortKeys4 ? kSortKeys4 : kSortKeys16;
  a.gs = std::min(cols, K >> a.log2c);
  const dim3 grid(slots, n, (cols + a.gs - 1) / a.gs);
  if (K == kSortKeys1)
    hipLaunchKernelGGL((quant_sort_kernel<1, kSortKeys1>), grid, dim3(64), 0, stream, a);
  else if (K == kSortKeys4)
    hipLaunchKernelGGL((quant_sort_kernel<4, kSortKeys4>), grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((quant_sort_kernel<16, kSortKeys16>), grid, dim3(1024), 0, stream, a);
}

// One export over a set's rings: ring(i, &R) fills base / stride / cols / mask / head / n and
// returns the ring's first series.
template <class Ring>
int export_rings(size_t nrings, uint32_t window, uint32_t P, float p0, float p1, float p2, float* dst, hipStream_t stream,
                 Ring ring) {
  QuantArgs a{};
  a.P = P;
  a.log2c = log2u(window / P);
  set_pct(a, p0, p1, p2);
  uint32_t n = 0;
  for (size_t i = 0; i < nrings; ++i) {
    QuantRing& R = a.r[n];
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

int launch_quantile_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                         uint32_t P, uint32_t rows_per_col, float p0, float p1, float p2, float* dst, void* stream_ptr) {
  if (bad_columns(P) || bad_dst(dst) || bad_pct(p0, p1, p2) || base == nullptr || !pow2(depth) || rows_per_col < 1 ||
      rows_per_col > kMaxTrendRowsPerColumn || depth % rows_per_col != 0 || n > depth || n > head ||
      uint64_t(n) > uint64_t(P) * rows_per_col || stride < 1 || stride > kMaxTrendStride || cols < 1 || cols > stride)
    return hipErrorInvalidValue;
  QuantArgs a{};
  a.P = P;
  a.log2c = log2u(rows_per_col);  // a divisor of a power of two
  set_pct(a, p0, p1, p2);
  a.r[0] = QuantRing{base, dst, head, stride, cols, depth - 1, n};
  launch(a, 1, static_cast<hipStream_t>(stream_ptr));
  return hipGetLastError();
}

// DeviceWindowSet::export_quantiles lives here with its kernel (device_window.h declares it);
// the window is export_trend's (window_trend.hip)
int DeviceWindowSet::export_quantiles(uint32_t P, float p0, float p1, float p2, float* dst, void* stream_ptr) const {
  if (bad_columns(P) || P > window_ || window_ / P > kMaxTrendRowsPerColumn || bad_dst(dst) || bad_pct(p0, p1, p2))
    return hipErrorInvalidValue;
  for (const auto& r : rings_)
    if (r.ring->width() > kMaxTrendStride) return hipErrorInvalidValue;
  DeviceScope scope(device_);
  return export_rings(rings_.size(), window_, P, p0, p1, p2, dst, static_cast<hipStream_t>(stream_ptr),
                      [&](size_t i, QuantRing& R) {
                        const auto& r = rings_[i];
                        R.base = r.dev;
                        R.stride = R.cols = r.ring->width();
                        R.mask = uint32_t(dev_rows() - 1);
                        R.head = r.state_valid ? r.last_head : 0;
                        R.n = r.state_valid ? r.last_n : 0;
                        return r.first_series;
                      });
}

// LongWindowSet::export_quantiles: rows [copied - min(copied, W), copied), as export_trend
int LongWindowSet::export_quantiles(uint32_t P, float p0, float p1, float p2, float* dst, void* stream_ptr) {
  if (bad_columns(P) || P > window_ || window_ / P > kMaxTrendRowsPerColumn || bad_dst(dst) || bad_pct(p0, p1, p2))
    return hipErrorInvalidValue;
  if (ingest_pending_) return hipErrorNotReady;  // staged rows no kernel has written yet: refresh() first
  DeviceScope scope(device_);
  return export_rings(rings_.size(), window_, P, p0, p1, p2, dst, static_cast<hipStream_t>(stream_ptr),
                      [&](size_t i, QuantRing& R) {
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
