// Host-side planning of the window cross-correlation (window_xcorr.h): which ring a pair lives
// in, how a pair becomes two directed items, which thread owns which lags of which item, where
// a lag of an item lands in the output, and how the chunks of a span are shared among the
// workgroups. No HIP in here: the kernel (window_xcorr.hip) and a host-only check under
// sanitizers (tools/xcorr_plan_check.cpp) compile the same text.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ROCMDASH_XCORR_HD __host__ __device__
#else
#define ROCMDASH_XCORR_HD
#endif

namespace rocmdash {

constexpr uint32_t kMaxXcorrPairs = 8;
constexpr uint32_t kXcorrWords = 6;           // n, Sx, Sy, Sxy, Sxx, Syy
constexpr uint32_t kXcorrGroupPairs = 4;      // pairs of a workgroup: 8 LDS rows, 8 directed items
constexpr uint32_t kXcorrLagBlock = 256;      // lags of a workgroup
constexpr uint32_t kXcorrLagTile = 8;         // consecutive lags a thread owns
constexpr uint32_t kXcorrThreads = 256;       // 8 items x 32 tiles
constexpr uint32_t kXcorrTargetGroups = 1024; // workgroups of a launch: two rounds of 2 per CU
constexpr uint32_t kMaxXcorrStride = 64;      // floats per ring row
constexpr uint32_t kXcorrChunk = 1024;        // rows of a chunk: the autocorrelation's
constexpr uint32_t kMaxXcorrLags = 1024;      // L: the autocorrelation's
constexpr uint32_t kXcorrPitch = kXcorrChunk + kMaxXcorrLags + 16;  // words of an LDS row: chunk, halo, the last read's reach
static_assert(2 * kXcorrGroupPairs * (kXcorrLagBlock / kXcorrLagTile) == kXcorrThreads, "one (item, tile) per thread");

// ---- pairs onto rings --------------------------------------------------------------------
struct XcorrRingSpan {
  uint32_t first_series, width;  // the ring's series are [first_series, first_series + width)
};

// The pairs of one ring, as the kernel takes them: columns of the ring and the output slot k
// of each. A pair named twice is summed twice, once per slot.
struct XcorrRingPairs {
  uint32_t ring = 0, count = 0;
  uint8_t a[kMaxXcorrPairs] = {}, b[kMaxXcorrPairs] = {}, slot[kMaxXcorrPairs] = {};
};

struct XcorrPlan {
  XcorrRingPairs rings[kMaxXcorrPairs];  // only rings with pairs, in ring order
  uint32_t nrings = 0;
};

// pairs: [K][2] series indices of the set. False - nothing usable in *plan - unless
// 1 <= K <= 8 and every pair has a != b, both below the set's series and both in one ring of
// at most 64 series.
inline bool xcorr_plan_pairs(const uint32_t* pairs, uint32_t K, const XcorrRingSpan* spans, uint32_t nspans, XcorrPlan* plan) {
  *plan = XcorrPlan{};
  if (pairs == nullptr || K < 1 || K > kMaxXcorrPairs) return false;
  int32_t ring_of[kMaxXcorrPairs];
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t a = pairs[2 * k], b = pairs[2 * k + 1];
    if (a == b) return false;
    int32_t ra = -1, rb = -1;
    for (uint32_t r = 0; r < nspans; ++r) {
      if (a >= spans[r].first_series && a - spans[r].first_series < spans[r].width) ra = int32_t(r);
      if (b >= spans[r].first_series && b - spans[r].first_series < spans[r].width) rb = int32_t(r);
    }
    if (ra < 0 || rb < 0 || ra != rb) return false;  // beyond the set, or a pair across rings
    if (spans[ra].width > kMaxXcorrStride) return false;
    ring_of[k] = ra;
  }
  for (uint32_t r = 0; r < nspans; ++r) {
    XcorrRingPairs p;
    p.ring = r;
    for (uint32_t k = 0; k < K; ++k) {
      if (ring_of[k] != int32_t(r)) continue;
      p.a[p.count] = uint8_t(pairs[2 * k] - spans[r].first_series);
      p.b[p.count] = uint8_t(pairs[2 * k + 1] - spans[r].first_series);
      p.slot[p.count] = uint8_t(k);
      ++p.count;
    }
    if (p.count) plan->rings[plan->nrings++] = p;
  }
  return true;
}

// ---- directed items, lag blocks and threads ----------------------------------------------
// Pair i of a ring's list sits in workgroup group i / 4 as LDS rows 2 (i % 4) (series a) and
// 2 (i % 4) + 1 (series b). Directed item r of the group has x = row r and y = row r ^ 1 and sums
// x[t] against y[t + k], k >= 0: an even r is (a, b) at lags k >= 0, an odd r is (b, a), which is
// (a, b) at lag -k.
ROCMDASH_XCORR_HD inline uint32_t xcorr_pair_groups(uint32_t count) { return (count + kXcorrGroupPairs - 1) / kXcorrGroupPairs; }
ROCMDASH_XCORR_HD inline uint32_t xcorr_group_rows(uint32_t count, uint32_t group) {
  const uint32_t left = count - group * kXcorrGroupPairs;
  return 2u * (left < kXcorrGroupPairs ? left : kXcorrGroupPairs);
}
// lags 0 .. L in blocks of 256: L = 256 m - 1 fills its blocks; at L = 256 m the last holds lag L alone
ROCMDASH_XCORR_HD inline uint32_t xcorr_lag_blocks(uint32_t L) { return L / kXcorrLagBlock + 1; }
ROCMDASH_XCORR_HD inline uint32_t xcorr_block_hi(uint32_t L, uint32_t block) {
  const uint32_t hi = block * kXcorrLagBlock + kXcorrLagBlock - 1;
  return hi < L ? hi : L;
}
ROCMDASH_XCORR_HD inline uint32_t xcorr_block_tiles(uint32_t L, uint32_t block) {
  return (xcorr_block_hi(L, block) - block * kXcorrLagBlock) / kXcorrLagTile + 1;
}
// Thread tid of a workgroup with `rows` LDS rows and `tiles` tiles of lags: its directed item
// *r and its tile *tile; false for a thread without one.
ROCMDASH_XCORR_HD inline bool xcorr_thread(uint32_t tid, uint32_t rows, uint32_t tiles, uint32_t* r, uint32_t* tile) {
  const bool mine = tid < rows * tiles;
  *r = mine ? tid / tiles : 0u;
  *tile = mine ? tid % tiles : 0u;
  return mine;
}
// Rows of the span a workgroup whose highest lag is `hi` loads per chunk: the chunk, the halo
// and the reach of the last 16-word read, in whole 8-word blocks; at most kXcorrPitch.
ROCMDASH_XCORR_HD inline uint32_t xcorr_load_rows(uint32_t hi) { return (kXcorrChunk + hi + 16 + 7) & ~7u; }
// Index of the pair's [2L + 1] for lag k of directed item r, -1 where the item does not own it:
// lags beyond L, and lag 0 of the odd item - lag 0 is added once, by the even one.
ROCMDASH_XCORR_HD inline int32_t xcorr_index(uint32_t L, uint32_t r, uint32_t k) {
  if (k > L || ((r & 1u) && k == 0)) return -1;
  return (r & 1u) ? int32_t(L - k) : int32_t(L + k);
}

// ---- shares ------------------------------------------------------------------------------
// `chunks` chunks among about kXcorrTargetGroups workgroups of `per_chunk` (pair groups x lag
// blocks) each: workgroup g of the x dimension takes chunks [g x share, min((g + 1) x share, chunks)).
ROCMDASH_XCORR_HD inline uint32_t xcorr_share(uint32_t chunks, uint32_t per_chunk) {
  uint32_t shares = kXcorrTargetGroups / (per_chunk ? per_chunk : 1u);
  if (shares < 1) shares = 1;
  if (shares > chunks) shares = chunks;
  return shares ? (chunks + shares - 1) / shares : 1u;
}
ROCMDASH_XCORR_HD inline uint32_t xcorr_share_groups(uint32_t chunks, uint32_t share) { return (chunks + share - 1) / share; }

}  // namespace rocmdash
