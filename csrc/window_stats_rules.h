// The pure rules of the window-stats kernel (window_stats.hip): integer and fp64
// arithmetic with no HIP runtime dependency beyond the qualifiers. The kernel, the host
// that predicts its path (device_window.cpp) and the CPU tests (through bindings.cpp,
// tests/test_window_stats_rules.py) all run these same functions.
#pragma once

#include <cmath>
#include <cstdint>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace rocmdash {

// Samples that may enter (and leave) a window between two refreshes for the
// incremental path; more than this falls back to a full sort.
constexpr int kMaxIncremental = 256;

// ---- path selection -------------------------------------------------------------
// Whether a launch over window [h1 - n1, h1) can update, incrementally, the state a
// previous launch left for window [h0 - n0, h0) in half `cur`: the window only moved
// forwards, by at most kMaxIncremental rows at either end, the leaving rows are still
// in the device ring (`depth` rows deep) and both windows fit a half of the resident
// buffer. `kadd` rows entered, `krem` left.
struct IncStep {
  bool ok;
  uint32_t kadd, krem;
};
__host__ __device__ constexpr IncStep incremental_step(uint64_t h0, uint32_t n0, uint32_t cur, uint64_t h1, uint32_t n1,
                                                       uint64_t depth, uint32_t sorted_cap) {
  if (h1 >= h0 && n0 <= h0 && cur <= 1) {
    const uint64_t s0 = h0 - n0, s1 = h1 - n1;
    if (s1 >= s0 && h1 - h0 <= uint64_t(kMaxIncremental) && s1 - s0 <= uint64_t(kMaxIncremental) && s0 + depth >= h1 &&
        n0 <= sorted_cap && n1 <= sorted_cap)
      return {true, uint32_t(h1 - h0), uint32_t(s1 - s0)};
  }
  return {false, 0u, 0u};
}

// The half of the resident buffer a launch leaves current: the incremental path updates
// half `cur` in place (a fall-back from it keeps `cur` too: its sort does not read the
// resident window); a full sort (first refresh or rebuild) writes the other half, or
// half 0 without state.
__host__ __device__ constexpr uint32_t next_half(bool incremental, bool have_state, uint32_t cur) {
  return incremental ? cur : (have_state ? (cur ^ 1u) : 0u);
}

// ---- what an incremental step changes ---------------------------------------------
// Only positions [lo, hi) of the new window (nv samples) can differ from the old one:
// below the first change point nothing moved, and with as many samples in as out
// nothing moved past the last one either. Leaving samples sit at old positions
// first_leave .. last_leave (read only if kr), entering ones go in before old positions
// first_ins .. last_ins (read only if ka).
struct Span {
  uint32_t lo, hi;
};
__host__ __device__ constexpr Span changed_span(uint32_t kr, uint32_t ka, uint32_t first_leave, uint32_t last_leave,
                                                uint32_t first_ins, uint32_t last_ins, uint32_t nv) {
  uint32_t lo = kr ? first_leave : 0xFFFFFFFFu;
  if (ka && first_ins < lo) lo = first_ins;
  uint32_t hi = nv;
  if (kr == ka) {
    hi = kr ? last_leave + 1u : 0u;
    if (ka && last_ins > hi) hi = last_ins;
    if (hi > nv) hi = nv;
  }
  return {lo, hi};
}

// At most one sample out (kr, from old position `leave`) and one in (ka, before old
// position `ins`): the new window is the old one shifted by one around the entering
// sample. `x` = old position of the leaving sample, `pn` = new position of the entering
// one (~0 = none); every other new position p holds old element src(p), one of
// p - 1, p, p + 1.
struct OneRowMap {
  uint32_t x, pn;
  __host__ __device__ constexpr uint32_t src(uint32_t p) const {
    const uint32_t m = p - (pn < p ? 1u : 0u);  // kept-element index
    return m + (x <= m ? 1u : 0u);
  }
};
__host__ __device__ constexpr OneRowMap one_row_map(uint32_t kr, uint32_t ka, uint32_t leave, uint32_t ins) {
  const uint32_t x = kr ? leave : 0xFFFFFFFFu;
  return {x, ka ? ins - (x < ins ? 1u : 0u) : 0xFFFFFFFFu};
}

// ---- outputs --------------------------------------------------------------------
// Sorted positions the outputs need: [min, max, lo0, hi0, lo1, hi1, lo2, hi2], and the
// three percentiles' fractions between their lo and hi (numpy's 'linear' definition).
__host__ __device__ inline void wanted_positions(uint32_t nv, const double qfrac[3], uint32_t (&idx)[8], float (&frac)[3]) {
  const uint32_t last = nv ? nv - 1 : 0;
  idx[0] = 0;
  idx[1] = last;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double pos = qfrac[q] * double(last);  // qfrac = double(pct) / 100, host-computed
    uint32_t lo = uint32_t(floor(pos));
    if (lo > last) lo = last;
    idx[2 + 2 * q] = lo;
    idx[3 + 2 * q] = lo + 1 < nv ? lo + 1 : last;
    frac[q] = float(pos - double(lo));
  }
}

// The percentile between order statistics x0 (at lo) and x1 (at hi).
__host__ __device__ inline float percentile_between(double x0, double x1, float frac) {
  const double f = frac;
  return float(f >= 0.5 ? x1 - (x1 - x0) * (1.0 - f) : x0 + (x1 - x0) * f);
}

// ---- sizes ----------------------------------------------------------------------
// Smallest supported sort width for a window of n samples.
__host__ __device__ constexpr uint32_t sort_width_for(uint32_t n) {
  uint32_t p = 64;
  while (p < n) p <<= 1;
  return p;
}

// Padded LDS layout of the old window in the incremental path: 4 spare floats after
// every 2^PS. With PS = log2(E) a thread's blocked E-float chunk sits E + 4 floats from
// its neighbour's, an odd multiple of 16 B for E >= 8: the 8 lanes of each group of a
// ds_write_b128 cover all 32 banks (no conflict), and float4 runs stay 16-byte aligned.
__host__ __device__ constexpr int pad_shift(int E) { return E >= 32 ? 5 : E >= 16 ? 4 : E >= 8 ? 3 : 6; }
__host__ __device__ constexpr uint32_t padded_size(uint32_t n, int ps) { return n + ((n >> ps) << 2) + 4; }
// Layout of the merged window in the walk path: 1 spare float after every 16, so the
// blocked scatter (lanes ~16 floats apart) hits 32 distinct banks with ds_write_b32.
__host__ __device__ constexpr uint32_t padded2_size(uint32_t n) { return n + (n >> 4) + 1; }

// Bits that hold a count in [0, E].
__host__ __device__ constexpr int count_bits(int e) { return e <= 1 ? 1 : 1 + count_bits(e >> 1); }

// ---- launch configuration -------------------------------------------------------
// Threads per workgroup and samples per thread (nt * e = the sort width) of the launch
// for sort width `pad_pow2`; nt = 0: unsupported width.
// Steady state (`incremental`: every series is expected to take the incremental path,
// 256 < width <= 8192): with at most one row in (the one-row path) 512 threads - two
// waves per SIMD overlap each other's dependent instructions - measured fastest; the
// general merge of k > 1 rows gains from 1024 (HIP events, W = 4096 x 15: k = 1 8.5 vs
// 9.1 us at 512 vs 1024 threads, k = 10 15.4 vs 14.0 us; profiles/r02/onerow/). (A
// series whose state turns out invalid still sorts correctly, with E = P / NT.)
// Free-running sampling brings 2 rows of the faster source into many refreshes: the
// series with one row keep the one-row path, those with two take the general path at
// 512 threads - hence `small_k`, the most entering rows that still count as few.
// With the SMU table tracked (sources.h) the amd-smi ring brings 4-6 rows a refresh and
// the launch is the 1024-thread one, the fifth and older rows pulled from the host ring.
// `small_k` stays 2: with 8 (512 threads at that mix) the refresh's device part measured
// 21.0-22.0 us against 20.4-20.5. Eight inline rows instead of kInlineRows = 4 (no pull
// at that mix, a 2.4 KiB kernel argument) measured 20.1-20.7 against 20.2-20.9 us over
// eight alternating rounds - no difference, not adopted (profiles/smu_track/).
// Otherwise (first refresh, stateless): as many threads as the width, at most 1024.
struct LaunchShape {
  int nt, e;
};
__host__ __device__ constexpr LaunchShape launch_shape(uint32_t pad_pow2, bool incremental, uint32_t max_new_rows,
                                                       uint32_t small_k) {
  if (pad_pow2 < 64 || pad_pow2 > 32768 || (pad_pow2 & (pad_pow2 - 1))) return {0, 0};
  int nt = pad_pow2 < 1024 ? int(pad_pow2) : 1024;
  if (incremental && pad_pow2 > 256 && pad_pow2 <= 8192)
    nt = pad_pow2 <= 1024 ? 256 : (pad_pow2 <= 2048 || max_new_rows <= small_k) ? 512 : 1024;
  return {nt, int(pad_pow2) / nt};
}

}  // namespace rocmdash
