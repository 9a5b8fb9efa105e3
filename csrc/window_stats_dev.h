// Device primitives of the window-stats kernel (window_stats.hip; node_window.hip takes
// its bound searches from here): the compare-exchange network, the bound searches, the
// wave sums, the series view and its sample accessor. Everything has internal linkage
// (an anonymous namespace per including file): the kernel has no LDS to spare for what
// external linkage costs.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "window_stats.h"

namespace rocmdash {
namespace {

// ---- compare-exchange network -----------------------------------------------------
// Stages of an ascending bitonic sort over values held E per thread, blocked layout:
// a[e] has sort position pos0 + e, pos0 = E * (the thread's index in the sort). Merge
// size k, partner distance j.
// Partner in the same wave64 (E <= j < 64 E): lane xor j / E through __shfl_xor.
template <int E>
__device__ __forceinline__ void cx_in_wave(float (&a)[E], uint32_t k, uint32_t j, uint32_t pos0) {
  const int m = int(j / E);
  const bool keep_min = ((pos0 & j) == 0) == ((pos0 & k) == 0);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float w = __shfl_xor(a[e], m);
    a[e] = keep_min ? fminf(a[e], w) : fmaxf(a[e], w);
  }
}

// Partner in the same thread (every j < E, j < k): compile-time register pairs.
template <int E>
__device__ __forceinline__ void cx_in_thread(float (&a)[E], uint32_t k, uint32_t pos0) {
#pragma unroll
  for (int jj = E / 2; jj >= 1; jj >>= 1) {
    if (uint32_t(jj) < k) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if ((e & jj) == 0) {
          const int f = e | jj;
          const bool asc = ((pos0 + e) & k) == 0;
          const float lo = fminf(a[e], a[f]);
          const float hi = fmaxf(a[e], a[f]);
          a[e] = asc ? lo : hi;
          a[f] = asc ? hi : lo;
        }
      }
    }
  }
}

// Ascending bitonic sort of 64*E values held E per lane, blocked layout
// (sort index = lane * E + e); registers and cross-lane shuffles only.
template <int E>
__device__ inline void wave_sort(float (&a)[E], int lane) {
  const uint32_t pos0 = uint32_t(lane) * E;
#pragma unroll
  for (uint32_t k = 2; k <= 64u * E; k <<= 1) {
    for (uint32_t j = k >> 1; j >= uint32_t(E); j >>= 1) cx_in_wave<E>(a, k, j, pos0);
    cx_in_thread<E>(a, k, pos0);
  }
}

// ---- searches -----------------------------------------------------------------------
// Index maps of the padded LDS layouts (window_stats_rules.h).
template <int PS>
__device__ __forceinline__ uint32_t pad(uint32_t i) { return i + ((i >> PS) << 2); }
__device__ __forceinline__ uint32_t pad2(uint32_t i) { return i + (i >> 4); }
struct AsIs {
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return i; }
};
template <int PS>
struct Padded {
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return pad<PS>(i); }
};

// First position in [lo, hi) of the ascending a[map(.)] whose element is > x (Upper)
// or >= x (lower), hi if none.
template <bool Upper, class T, class Map = AsIs>
__device__ inline uint32_t bound(const T* a, uint32_t lo, uint32_t hi, T x, Map map = Map{}) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const T v = a[map(mid)];
    if (Upper ? v <= x : v < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// 64-ary upper_bound by a whole wave over an ascending (padded) LDS array: each round
// every lane tests one pivot and a ballot narrows the range 64-fold; the result is uniform.
template <int PS>
__device__ inline uint32_t wave_upper_bound(const float* a, uint32_t n, float x, int lane) {
  uint32_t lo = 0, len = n;
  while (len > 64) {
    uint32_t step = (len + 63) / 64;
    step += (step & 7u) == 0 ? 1u : 0u;  // pivots a multiple of 8 apart would share 2 LDS banks
    const uint32_t i = lo + uint32_t(lane) * step;
    const bool before = i < lo + len && a[pad<PS>(i)] <= x;
    const uint32_t c = __popcll(__ballot(before));  // chunks whose first element is <= x
    if (c == 0) return lo;
    const uint32_t end = lo + len;
    lo += (c - 1) * step;
    len = (lo + step < end ? lo + step : end) - lo;
  }
  const bool before = uint32_t(lane) < len && a[pad<PS>(lo + lane)] <= x;
  return lo + __popcll(__ballot(before));
}

// ---- wave sums ------------------------------------------------------------------------
// Wave64 sums through DPP (VALU lane moves, no LDS pipeline): xor 1 and xor 2 inside
// each quad, the half-row and row mirrors, so every lane of a 16-lane row holds the row
// sum; the four row sums are then read from lanes 0 / 16 / 32 / 48. (The shuffles they
// replace were ds_bpermute round trips, 12 dependent ones for one double.)
template <int Ctrl>
__device__ __forceinline__ double dpp_f64(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const int lo = __builtin_amdgcn_update_dpp(0, int(uint32_t(u)), Ctrl, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, int(uint32_t(u >> 32)), Ctrl, 0xF, 0xF, false);
  return __builtin_bit_cast(double, uint64_t(uint32_t(lo)) | (uint64_t(uint32_t(hi)) << 32));
}

__device__ inline double wave_sum(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp_f64<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp_f64<0x141>(v);  // row_half_mirror
  v += dpp_f64<0x140>(v);  // row_mirror
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  double r = 0.0;
#pragma unroll
  for (int row = 0; row < 4; ++row) {
    const uint32_t lo = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(u)), 16 * row));
    const uint32_t hi = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(u >> 32)), 16 * row));
    r += __builtin_bit_cast(double, uint64_t(lo) | (uint64_t(hi) << 32));
  }
  return r;
}

__device__ inline uint32_t wave_sum(uint32_t v) {
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0xB1, 0xF, 0xF, false));
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x4E, 0xF, 0xF, false));
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x141, 0xF, 0xF, false));
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x140, 0xF, 0xF, false));
  return uint32_t(__builtin_amdgcn_readlane(int(v), 0)) + uint32_t(__builtin_amdgcn_readlane(int(v), 16)) +
         uint32_t(__builtin_amdgcn_readlane(int(v), 32)) + uint32_t(__builtin_amdgcn_readlane(int(v), 48));
}

// ---- the series and its samples ------------------------------------------------------
// The series state through the vector memory path (a buffer load into VGPRs). A plain
// load of this uniform address becomes a scalar load whose SGPRs the compiler spills
// to VGPR lanes at once - waiting for the load right there, before the incremental
// path's own loads could go out; in VGPRs it is first waited for where it is used.
__device__ inline SeriesState load_state_vmem(const SeriesState* p) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<SeriesState*>(p), 0, int(sizeof(SeriesState)), 0x00020000);
  const auto a = __builtin_amdgcn_raw_buffer_load_b128(r, 0, 0, 0);  // head (lo, hi), n, nvalid
  const auto b = __builtin_amdgcn_raw_buffer_load_b64(r, 16, 0, 0);   // cur, valid
  SeriesState s;
  s.head = uint64_t(a[0]) | (uint64_t(a[1]) << 32);
  s.n = a[2];
  s.nvalid = a[3];
  s.cur = b[0];
  s.valid = b[1];
  return s;
}

// One series as the kernel sees it: its ring's head, with `sorted`, `state` and
// `n_inline` narrowed to its column, + the column itself.
struct SeriesView : RingHead {
  const float* inl;  // &ring.inl[0][col]; row r at inl[r * kMaxInlineWidth]
  uint32_t col;
};

// The workgroup of column `col` of ring `ri` (blockIdx.x, blockIdx.y): its ring's
// fields come from ONE round of scalar loads at an offset known at launch - no kernarg
// load waits for another (a series -> ring search over the rings' column counts did:
// two dependent kernel-argument round trips before the first global load).
__device__ inline SeriesView make_view(const StatsArgs& args, uint32_t ri, uint32_t col) {
  SeriesView v;
  static_cast<RingHead&>(v) = args.rings[ri].h;
  v.col = col;
  v.inl = &args.rings[ri].inl[0][0];  // indexed, not selected: keeps the kernarg a kernarg
  if (v.sorted) v.sorted += size_t(col) * 2 * v.sorted_cap;
  if (v.state) v.state += col;
  v.inl += col < uint32_t(kMaxInlineWidth) ? col : 0u;
  if (col >= uint32_t(kMaxInlineWidth)) v.n_inline = 0;
  return v;
}

// Row `row` of the series in the device ring.
__device__ __forceinline__ float& ring_sample(const SeriesView& d, uint64_t row) {
  return d.base[(row & d.mask) * d.stride + d.col];
}

// Where sample `row` of a series comes from: the newest rows travel by value in the
// kernel argument, older entering rows are in the pinned host ring in pull mode - both
// still have to go into the device ring, for the launch that later removes them - the
// rest is in the device ring the host filled with hipMemcpyAsync.
enum class Source { Inline, Host, Device };
__device__ __forceinline__ Source sample_source(const SeriesView& d, uint64_t row) {
  return row + d.n_inline >= d.head ? Source::Inline : d.host_rows != nullptr ? Source::Host : Source::Device;
}
__device__ __forceinline__ float inline_sample(const SeriesView& d, uint64_t row) {
  return d.inl[(row + d.n_inline - d.head) * kMaxInlineWidth];
}
__device__ __forceinline__ float host_sample(const SeriesView& d, uint64_t row) {
  return d.host_rows[(row & d.host_mask) * d.stride + d.col];
}

// Sample `row`, stored into the device ring where it has to be.
__device__ inline float take_sample(const SeriesView& d, uint64_t row) {
  float x;
  switch (sample_source(d, row)) {
    case Source::Inline: x = inline_sample(d, row); break;
    case Source::Host: x = host_sample(d, row); break;
    default: return ring_sample(d, row);
  }
  ring_sample(d, row) = x;
  return x;
}

// Sample `row` without storing it (every thread of the one-row path reads it; thread 0
// stores it): `store` tells whether it still has to go into the device ring.
__device__ inline float peek_sample(const SeriesView& d, uint64_t row, bool& store) {
  const Source s = sample_source(d, row);
  store = s != Source::Device;
  if (s == Source::Inline) return inline_sample(d, row);
  return s == Source::Host ? host_sample(d, row) : ring_sample(d, row);
}

}  // namespace
}  // namespace rocmdash
