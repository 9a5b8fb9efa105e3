// Window distributions as cumulative le-buckets: for each series, how many valid samples
// of its window are <= each of B upper bounds, + the valid count (the +Inf bucket) - the
// form of a distribution that sums across GPUs, nodes and scrapes (Prometheus `le`
// semantics: histogram_quantile(q, sum by (le) (...))).
//
// Every series' window is already sorted in HBM (the resident state of the window-stats
// kernel, window_stats.hip), so a bucket is ONE upper_bound in that array: B searches per
// series, no pass over the ring and nothing added to the stats kernel. One wave64 per
// series: lane b < B searches bound b, lane B writes the valid count, so 1 <= B <= 63.
// Counts are stored as float32 - exact, every count is < 2^24 - like element 0 of an
// export block (node_window.h).
//
// Two entries over the one device routine:
//   * DeviceWindowSet::export_buckets (device_window.h): over the resident sorted windows;
//   * launch_bucket_blocks: over export blocks [N][S][1 + W] (export_sorted's layout, what
//     the node-window gather moves), per rank and summed over the ranks.
#pragma once

#include <cstdint>

namespace rocmdash {

constexpr uint32_t kMaxBuckets = 63;          // finite bounds per series (lane B: the count)
constexpr uint32_t kMaxBucketRanks = 64;      // 64 x 32768 < 2^24: the node sum stays exact
constexpr int kBucketSeriesPerLaunch = 128;   // series refs in one export_buckets launch

// blocks: device [N][S][1 + W]; bounds: device [S][B], finite and strictly ascending per
// series; per_rank: device [N][S][B + 1] or nullptr; node: device [S][B + 1] (the sum over
// the N ranks) or nullptr. out[..][b] = samples <= bounds[s][b] (fp32 compare),
// out[..][B] = the valid count. Returns a hipError_t: hipErrorInvalidValue, before any
// launch, for B outside [1, 63], N > 64, W = 0 or a null blocks / bounds pointer.
int launch_bucket_blocks(const float* blocks, uint32_t N, uint32_t S, uint32_t W, const float* bounds, uint32_t B,
                         float* per_rank, float* node, void* stream);

}  // namespace rocmdash
