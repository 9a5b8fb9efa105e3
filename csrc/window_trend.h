// Window trend: every series' window decimated into a chart's worth of columns - per column
// {min, max, mean, count} of its rows - the one view of a window that keeps WHEN things
// happened (window_stats.h gives 8 scalars, window_buckets.h a distribution).
//
// Columns are anchored to absolute row numbers: with c rows per column, row r (rows ever
// written, 0-based) belongs to column r / c, so a full column never changes while the
// window slides over it. A window [head - n, head) of n <= P x c rows touches at most P + 1
// aligned columns: the output has P + 1 slots per series, slot j (0 = oldest, P = newest)
// being column (head - 1) / c - P + j cut to the window. c divides the ring depth, so a
// column is one contiguous, unwrapped block of c rows of the time-major device ring.
//
// Per (series, slot) one 16-byte store {min, max, mean, count}: NaN samples are skipped,
// min / max are selections by the order-preserving key (-0.0 < +0.0), the mean is every
// valid sample added in fp64 in a fixed order, divided in fp64 and rounded once, count is
// exact (<= 65536). A slot without a valid sample is {NaN, NaN, NaN, 0}.
//
// Three entries over the one device routine:
//   * launch_trend_ring: one ring of series described by value;
//   * DeviceWindowSet::export_trend (device_window.h): the device rings of the last refresh;
//   * LongWindowSet::export_trend (long_window.h): the long windows of the last refresh.
#pragma once

#include <cstdint>

namespace rocmdash {

constexpr uint32_t kMinTrendColumns = 8;
constexpr uint32_t kMaxTrendColumns = 1024;
constexpr uint32_t kMaxTrendRowsPerColumn = 65536;  // one workgroup's stream; the count stays exact in fp32
constexpr uint32_t kMaxTrendStride = 64;            // floats per ring row: a wave holds at least one row
constexpr int kTrendRingsPerLaunch = 8;

// base: device ring [depth][stride] floats, row r at slot r & (depth - 1), of which the first
// `cols` columns are series; the window is rows [head - n, head). dst: device
// [cols][P + 1][4] floats, 16-byte aligned. Returns a hipError_t: hipErrorInvalidValue,
// before any launch, unless P is a power of two in [8, 1024], depth a power of two,
// 1 <= rows_per_col <= 65536 divides depth, n <= depth, n <= head, n <= P x rows_per_col,
// 1 <= cols <= stride <= 64 and base / dst are set.
int launch_trend_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                      uint32_t P, uint32_t rows_per_col, float* dst, void* stream);

}  // namespace rocmdash
