// Window period trend: the autocorrelation's exact integer lag sums per trend column of a ring -
// each series' period over time. The semantics are stated once, in
// rocmdash/ops/window_periods.py: the newest n' = min(n, span) rows are cut into the trend's
// P + 1 slots for a window of `span` rows (columns of c = span / P rows anchored to absolute row
// numbers), and slot j with rows [b, e) holds the autocorrelation's four sums {n, Sx, Sy, Sxy}
// (window_autocorr.h: its quantisation, its scale) of those rows alone - a pair (t, t + k)
// counts only when b <= t and t + k < e. Output: int64 [S][P + 1][L + 1][4], every word
// written; an empty slot and every lag k >= e - b are zero. The period of a slot is host
// arithmetic on these integers.
//
// One launch per ring for all slots: grid (slots x split, groups of 8 series, blocks of 256
// lags), 256 threads, a thread owns 8 consecutive lags of one series. A workgroup walks its
// chunks of 1024 rows of one slot in order; per chunk the chunk and the halo its lags reach sit
// in LDS as 16-bit words [series][chunk + halo] (q, bit 15 = invalid), rows at and beyond the
// slot's end stored as invalid with q = 0, so the autocorrelation's prefix-sum path for a clean
// series and its two walks for one with a NaN carry over with the rows left measured to the
// slot's end. With split == 1 the workgroup owns its (slot, series group, lag block) and writes
// every lag's four words with two plain 16-byte stores, zeroes included: no memset, no atomic,
// no workspace. With split > 1 (window_periods_plan.h decides) a slot's chunks are shared among
// `split` workgroups, the destination is zeroed in stream order and the non-zero sums are added
// with vector 64-bit integer atomics, as the autocorrelation does. Both are one device routine,
// the epilogue a template flag. As compiled for gfx950 (ROCm 7.2.0), either epilogue: 41376 bytes
// of LDS per workgroup (the words of 8 series x 2064 rows, their block prefixes), 184 VGPRs, no
// scratch - 2 waves per SIMD, two workgroups of 4 waves share a CU.
//
// Three entries over the one device routine:
//   * launch_periods_ring: one ring of series described by value;
//   * DeviceWindowSet::export_periods (device_window.h): the device rings of the last refresh;
//   * LongWindowSet::export_periods (long_window.h): the long windows of the last refresh.
#pragma once

#include <cstdint>

#include "window_autocorr.h"

namespace rocmdash {

constexpr uint32_t kMinPeriodsSpan = 1u << 9;  // span, a power of two
constexpr uint32_t kMaxPeriodsSpan = kMaxAutocorrSpan;
constexpr uint32_t kMinPeriodsColumns = 8;  // P, a power of two
constexpr uint32_t kMaxPeriodsColumns = 64;
constexpr uint32_t kMinPeriodsRowsPerColumn = 64;  // c = span / P
constexpr uint32_t kMaxPeriodsRowsPerColumn = 65536;
constexpr uint32_t kMaxPeriodsWords = 16384;  // P x (L + 1): the output of a series

inline bool bad_periods(uint32_t span, uint32_t P, const float* scale, uint32_t L, const int64_t* dst) {
  if (span < kMinPeriodsSpan || span > kMaxPeriodsSpan || (span & (span - 1)) != 0) return true;
  if (P < kMinPeriodsColumns || P > kMaxPeriodsColumns || (P & (P - 1)) != 0) return true;
  const uint32_t c = span / P;
  if (c < kMinPeriodsRowsPerColumn || c > kMaxPeriodsRowsPerColumn) return true;
  if (L < 1 || L > kMaxAutocorrLags || 2 * L > c || uint64_t(P) * (L + 1) > kMaxPeriodsWords) return true;
  return scale == nullptr || dst == nullptr || (reinterpret_cast<uintptr_t>(dst) & 15u) != 0;
}

// base / stride / cols / depth / head / n as launch_autocorr_ring; the rows are the newest
// min(n, span) of the window. scale: device [cols] floats, finite and > 0. dst:
// device [cols][P + 1][L + 1][4] int64, 16-byte aligned, needs no initialisation. n == 0 or
// head == 0: all zeroes. split: 0 lets the plan decide; otherwise the workgroups that share a
// slot's chunks, a power of two no larger than the chunks of a full slot. Returns a hipError_t:
// hipErrorInvalidValue, before any launch or write, unless span is a power of two in
// [2^9, 2^20], P one in [8, 64], 64 <= span / P <= 65536, 1 <= L <= min(1024, span / P / 2),
// P (L + 1) <= 16384, the ring conditions hold, the split is one the plan takes and base / scale
// / dst are set.
int launch_periods_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                        uint32_t span, uint32_t P, const float* scale, uint32_t L, int64_t* dst, uint32_t split, void* stream);

}  // namespace rocmdash
