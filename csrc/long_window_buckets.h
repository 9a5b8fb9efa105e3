// Cumulative le-buckets of windows that keep no sorted state: the counts of window_buckets.h
// (valid samples <= each of B upper bounds, then the valid count), streamed from the
// time-major device rings - the long windows of LongWindowSet, 2^10 to 2^26 rows.
//
// One pass over the window, the stream of window_trend.hip with an integer reduction: many
// workgroups each take a contiguous share of the window's floats, a lane stays on one series
// and bins each valid sample by #{b : bounds[b] < x} (a histogram of B + 1 bins, counters in
// LDS), the workgroups add their non-zero bins onto the destination with vector global
// atomics, and a small second kernel turns every series' bins into cumulative counts.
// Integer adds: exact, and the same bits in any order.
//
// Counts are stored as float64: a long window holds up to 2^26 samples and a node sums 8
// of them, past the 2^24 up to which fp32 is exact. They are accumulated in uint32 (every
// count is <= 2^26) in the low words of the destination's own doubles, zeroed in stream
// order first: no scratch memory, nothing allocated.
//
// Semantics as window_buckets.h: fp32 compare, ties count, -0.0 == +0.0, -inf is in every
// bucket, +inf only in the last, NaN is skipped.
//
// Two entries over the one device routine:
//   * launch_bucket_ring: one ring of series described by value;
//   * LongWindowSet::export_buckets (long_window.h): the long windows of the last refresh.
#pragma once

#include <cstdint>

namespace rocmdash {

constexpr uint32_t kMaxBucketStride = 64;  // floats per ring row: a wave holds at least one row
constexpr int kBucketRingsPerLaunch = 8;

// base: device ring [depth][stride] floats, row r at slot r & (depth - 1), of which the first
// `cols` columns are series; the window is rows [head - n, head). bounds: device [cols][B],
// finite and strictly ascending per series (a ring of a set passes the row of its first
// series). dst: device [cols][B + 1] doubles. n == 0 or head == 0: all-zero counts. Returns a
// hipError_t: hipErrorInvalidValue, before any launch or write, unless 1 <= B <= 63, depth
// is a power of two, n <= depth, n <= head, 1 <= cols <= stride <= 64 and base / bounds /
// dst are set (dst 8-byte aligned).
int launch_bucket_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                       const float* bounds, uint32_t B, double* dst, void* stream);

}  // namespace rocmdash
