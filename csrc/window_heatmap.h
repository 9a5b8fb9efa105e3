// Window heatmap: per column of the window trend (window_trend.h) the le-bucket bins of the
// long buckets (long_window_buckets.h) - the distribution over time, the one view neither
// keeps. The semantics are stated once, in rocmdash/ops/window_heatmap.py: the slots are the
// trend's P + 1, a valid sample x of series s falls in bin #{b : bounds[s][b] < x} (fp32),
// NaN is skipped, and the output is int32 [series][P + 1][B + 1] of per-bin counts (not
// cumulative; each <= 65536; an empty slot is all zeroes).
//
// A slot is one contiguous, unwrapped block of the time-major device ring and is owned by
// exactly one wave or one workgroup, which counts it in LDS and then writes every (series,
// bin) of it with a plain store, zeroes included: no global atomics, no zeroing pass, no
// finalize kernel, no workspace, and the same bits on every run.
//
// Three entries over the one device routine:
//   * launch_heatmap_ring: one ring of series described by value;
//   * DeviceWindowSet::export_heatmap (device_window.h): the device rings of the last refresh;
//   * LongWindowSet::export_heatmap (long_window.h): the long windows of the last refresh.
#pragma once

#include <cstdint>

namespace rocmdash {

constexpr int kHeatmapRingsPerLaunch = 8;

// base / stride / cols / depth / head / n / P / rows_per_col as launch_trend_ring
// (window_trend.h); bounds: device [cols][B] as launch_bucket_ring (long_window_buckets.h: a
// ring of a set passes the row of its first series); dst: device [cols][P + 1][B + 1] int32,
// 4-byte aligned, needs no initialisation. Returns a hipError_t: hipErrorInvalidValue, before
// any launch or write, unless launch_trend_ring's conditions hold, 1 <= B <= 63 and base /
// bounds / dst are set.
int launch_heatmap_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                        uint32_t P, uint32_t rows_per_col, const float* bounds, uint32_t B, int32_t* dst, void* stream);

}  // namespace rocmdash
