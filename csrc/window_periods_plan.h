// Host-side planning of the window period trend (window_periods.h): the rows of a slot, the grid
// of a launch, whether a workgroup owns its whole slot or the slot's chunks are split among
// several, and which chunks each of those takes. No HIP in here: the kernel (window_periods.hip)
// and a host-only check under sanitizers (tools/periods_plan_check.cpp) compile the same text.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ROCMDASH_PERIODS_HD __host__ __device__
#else
#define ROCMDASH_PERIODS_HD
#endif

namespace rocmdash {

constexpr uint32_t kPeriodsChunk = 1024;         // rows of a chunk: the autocorrelation's
constexpr uint32_t kPeriodsSeriesGroup = 8;      // series of a workgroup
constexpr uint32_t kPeriodsLagBlock = 256;       // lags of a workgroup
constexpr uint32_t kPeriodsTargetGroups = 1024;  // workgroups of a launch: the autocorrelation's target

// Slot j (0 = oldest, P = newest) of the newest n rows [head - n, head), n <= span, in columns
// of c = span / P rows anchored to absolute row numbers: column (head - 1) / c - P + j cut to
// those rows - rocmdash.ops.window_trend.trend_geometry for a window of `span` rows. *b, *e: the
// slot's rows [b, e); false, with both 0, for an empty slot.
ROCMDASH_PERIODS_HD inline bool periods_slot(uint64_t head, uint32_t n, uint32_t c, uint32_t P, uint32_t j, uint64_t* b,
                                             uint64_t* e) {
  *b = *e = 0;
  if (n == 0 || head == 0) return false;
  const uint64_t last = (head - 1) / c;
  if (last + j < P) return false;  // a column before row 0
  const uint64_t a = last + j - P, lo = head - n;
  const uint64_t b0 = a * c > lo ? a * c : lo, e0 = (a + 1) * c < head ? (a + 1) * c : head;
  if (b0 >= e0) return false;
  *b = b0;
  *e = e0;
  return true;
}

struct PeriodsPlan {
  uint32_t groups = 0;  // groups of 8 series: grid y
  uint32_t blocks = 0;  // blocks of 256 lags: grid z
  uint32_t chunks = 0;  // chunks of a full slot
  uint32_t split = 0;   // workgroups that share a slot's chunks; 1: owned; grid x = slots x split
};

ROCMDASH_PERIODS_HD inline bool periods_pow2(uint64_t x) { return x != 0 && (x & (x - 1)) == 0; }

// slots = P + 1, rows = c (rows of a full slot), cols series, lags 0 .. L. Owned (split 1) when
// the owned items alone reach the target or a slot has one chunk; otherwise the smallest power of
// two that reaches it, at most the chunks of a slot. split_override != 0 replaces the rule; false
// unless it is a power of two no larger than the chunks of a slot.
inline bool periods_plan(uint32_t slots, uint32_t rows, uint32_t cols, uint32_t L, uint32_t split_override, PeriodsPlan* plan) {
  PeriodsPlan p;
  p.groups = (cols + kPeriodsSeriesGroup - 1) / kPeriodsSeriesGroup;
  p.blocks = L / kPeriodsLagBlock + 1;  // L = 256 m - 1 fills its blocks; at L = 256 m the last holds lag L alone
  p.chunks = (rows + kPeriodsChunk - 1) / kPeriodsChunk;
  if (p.chunks < 1) p.chunks = 1;
  if (split_override != 0) {
    if (!periods_pow2(split_override) || split_override > p.chunks) return false;
    p.split = split_override;
  } else {
    const uint64_t owned = uint64_t(slots) * p.groups * p.blocks;
    p.split = 1;
    while (owned * p.split < kPeriodsTargetGroups && p.split * 2 <= p.chunks) p.split *= 2;
  }
  *plan = p;
  return true;
}

// The chunks [*c0, *c1) of a slot of `chunks` chunks (at most plan_chunks, those of a full slot)
// that part `part` of `split` takes: plan_chunks is shared evenly, a short slot leaves the last
// parts empty (*c0 == *c1).
ROCMDASH_PERIODS_HD inline void periods_chunk_range(uint32_t chunks, uint32_t plan_chunks, uint32_t split, uint32_t part,
                                                    uint32_t* c0, uint32_t* c1) {
  const uint32_t share = (plan_chunks + split - 1) / split;
  const uint32_t lo = part * share, hi = lo + share;
  *c0 = lo < chunks ? lo : chunks;
  *c1 = hi < chunks ? hi : chunks;
}

}  // namespace rocmdash
