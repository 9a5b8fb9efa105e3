// Window quantile trend: the three percentiles of every trend column (window_trend.h), exact.
//
// Columns and slots are the trend's: c = window / P rows per column, anchored to absolute row
// numbers, P + 1 slots per series, slot j being column (head - 1) / c - P + j cut to the
// window (rocmdash.ops.window_trend.trend_geometry is the one statement of them).
//
// Per (series, slot) one 16-byte store {p_a, p_b, p_c, count}: over the slot's valid (non-NaN)
// samples in key order (-0.0 < +0.0) the percentiles are the stats kernels' arithmetic, bit
// for bit - wanted_positions for lo / hi / frac with qfrac = double(float(pct)) / 100 computed
// on the host, then percentile_between(x0, x1, frac) (window_stats_rules.h). The six order
// statistics are selections; where the percentile is one of them (frac == 0 or x0 == x1) and
// it is infinite, it is returned as it is, not as the NaN the arithmetic makes of inf - inf.
// count is exact (<= 65536) and the trend's. A slot without a valid sample is
// {NaN, NaN, NaN, 0}.
//
// A workgroup owns a (ring, slot, group of series) and stores each of its outputs once: no
// global atomics, no workspace, no second kernel, and the same bits on every run. Two paths,
// picked by the rows per column alone:
//   * c <= kQuantileSortMaxRows: the slot's keys are sorted in LDS, every series' segment at
//     once (a bitonic network; c is a power of two), and the six positions read;
//   * above: an MSD radix select over LDS histograms - the workgroup streams its slot once for
//     min / max / count and once per 8-bit digit below the highest bit in which the slot's
//     keys differ.
//
// Three entries over the one device routine:
//   * launch_quantile_ring: one ring of series described by value;
//   * DeviceWindowSet::export_quantiles (device_window.h): the device rings of the last refresh;
//   * LongWindowSet::export_quantiles (long_window.h): the long windows of the last refresh.
#pragma once

#include <cstdint>

namespace rocmdash {

// the most rows per column the LDS sort takes; more rows per column are selected by radix
constexpr uint32_t kQuantileSortMaxRows = 4096;

// base / stride / cols / depth / head / n / P / rows_per_col / dst / stream: as
// launch_trend_ring (window_trend.h), with its argument checks; p0, p1, p2: the percentiles,
// each finite and in [0, 100]. Returns a hipError_t: hipErrorInvalidValue before any launch
// or write for a bad argument.
int launch_quantile_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                         uint32_t P, uint32_t rows_per_col, float p0, float p1, float p2, float* dst, void* stream);

}  // namespace rocmdash
