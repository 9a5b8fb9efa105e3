// The run-length monoid of the window excursions (window_excursions.h; the one statement of
// the semantics is rocmdash/ops/window_excursions.py, whose excursion_combine is this
// combine). Plain C++: no HIP builtins, so the kernels and a host-only program
// (tools/excursion_monoid_check.cpp) compile the same text.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ROCMDASH_EXC_HD __host__ __device__ inline
#else
#define ROCMDASH_EXC_HD inline
#endif

namespace rocmdash {

// A time range's partial for one threshold, lengths in valid samples. All zero = the empty
// range, the identity of excursion_combine.
struct ExcursionPartial {
  uint32_t len;         // valid samples
  uint32_t above;       // of them above the threshold
  uint32_t pre;         // the leading above run
  uint32_t suf;         // the trailing above run
  uint32_t longest;     // the longest above run
  uint32_t episodes;    // maximal above runs
  uint32_t tail_below;  // the trailing not-above run
};

// One more sample at the range's newest end: `valid` = not NaN, `above` = x > threshold.
// Selects only; an invalid sample changes nothing.
ROCMDASH_EXC_HD void excursion_push(ExcursionPartial& p, bool valid, bool above) {
  const bool up = valid && above, down = valid && !above;
  p.episodes += uint32_t(up && p.suf == 0);
  p.pre += uint32_t(up && p.pre == p.len);
  p.suf = up ? p.suf + 1 : (down ? 0u : p.suf);
  p.tail_below = down ? p.tail_below + 1 : (up ? 0u : p.tail_below);
  p.above += uint32_t(up);
  p.longest = p.longest > p.suf ? p.longest : p.suf;
  p.len += uint32_t(valid);
}

// `a` then `b`, adjacent in time: associative, not commutative. The formulas hold for an
// empty side as they stand (0 == 0 extends the other side's run by 0).
ROCMDASH_EXC_HD ExcursionPartial excursion_combine(const ExcursionPartial& a, const ExcursionPartial& b) {
  ExcursionPartial r;
  r.len = a.len + b.len;
  r.above = a.above + b.above;
  r.pre = a.pre == a.len ? a.len + b.pre : a.pre;
  r.suf = b.suf == b.len ? b.len + a.suf : b.suf;
  r.tail_below = b.tail_below == b.len ? b.len + a.tail_below : b.tail_below;
  const uint32_t joined = a.suf + b.pre;
  const uint32_t m = a.longest > b.longest ? a.longest : b.longest;
  r.longest = m > joined ? m : joined;
  r.episodes = a.episodes + b.episodes - uint32_t(a.suf > 0 && b.pre > 0);
  return r;
}

// The record of a whole window of `rows` rows (window_excursions.h lists the eight fields).
ROCMDASH_EXC_HD void excursion_record(const ExcursionPartial& p, uint32_t rows, int32_t out[8]) {
  out[0] = int32_t(p.above);
  out[1] = int32_t(p.len);
  out[2] = int32_t(p.episodes);
  out[3] = int32_t(p.longest);
  out[4] = int32_t(p.suf);
  out[5] = int32_t(p.tail_below);
  out[6] = int32_t(p.pre);
  out[7] = int32_t(rows);
}

}  // namespace rocmdash
