// Window joint histogram: two series of one ring binned together - how they move together,
// which no per-series output can tell (marginals do not determine a joint distribution). The
// semantics are stated once, in rocmdash/ops/window_joint.py: 1 to 8 ordered pairs (a, b) of
// series of the same ring, a != b; the bin of a sample is the long buckets' rule
// (long_window_buckets.h: #{k : bounds[s][k] < x} in fp32, 1 <= B <= 31); a row counts for a
// pair only when both its samples are not NaN; the output is int32 [K][B + 1][B + 1] with
// out[k][i][j] the rows of the window with bin(x_a) == i and bin(x_b) == j, every cell written.
//
// One pass over the time-major device ring, the stream of long_window_buckets.hip: a lane
// bins its own sample, the two bins of a pair - lanes of one wave, a few lanes apart - meet
// through a wave shuffle, and the lane that owns the (row, pair) counts the cell in a
// workgroup-shared LDS table. The destination is zeroed in stream order and the workgroups
// add their non-zero cells with vector global integer atomics: exact, and the same bits in
// any order. No workspace, nothing allocated.
//
// Three entries over the one device routine:
//   * launch_joint_ring: one ring of series described by value;
//   * DeviceWindowSet::export_joint (device_window.h): the device rings of the last refresh;
//   * LongWindowSet::export_joint (long_window.h): the long windows of the last refresh.
#pragma once

#include <cstdint>

#include "window_joint_plan.h"

namespace rocmdash {

// base / stride / cols / depth / head / n as launch_bucket_ring (long_window_buckets.h).
// pairs: HOST [K][2] columns of the ring, each < cols, a != b. bounds: device [cols][B].
// dst: device [K][B + 1][B + 1] int32, 4-byte aligned, needs no initialisation. n == 0 or
// head == 0: all zeroes. Returns a hipError_t: hipErrorInvalidValue, before any launch or
// write, unless 1 <= K <= 8, 1 <= B <= 31, the pairs are as above, launch_bucket_ring's ring
// conditions hold and base / pairs / bounds / dst are set.
int launch_joint_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                      const uint32_t* pairs, uint32_t K, const float* bounds, uint32_t B, int32_t* dst, void* stream);

}  // namespace rocmdash
