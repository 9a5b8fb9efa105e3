// Host-only check of csrc/window_periods_plan.h, the text the period trend kernel compiles: over
// a sweep of spans, columns, series counts and lag counts the plan must give a grid that owns
// every (series, lag) of a slot exactly once, a split that is a power of two no larger than the
// chunks of a slot and follows the stated rule, and chunk ranges that partition the chunks of
// every slot - full, short and empty - exactly once among the split's parts; over random heads
// and row counts the slots must partition the newest rows in order, each within one column; the
// refusals of a split override must refuse. Build with -fsanitize=address,undefined and run on
// the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc tools/periods_plan_check.cpp -o check && ./check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "window_periods_plan.h"

using namespace rocmdash;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::printf("FAILED %s: ", #cond);          \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
      std::exit(1);                               \
    }                                             \
  } while (0)

long checked_plans = 0, checked_ranges = 0, checked_slots = 0;

// every slot's chunks, whatever their number up to the plan's, go to the parts exactly once and in order
void check_ranges(const PeriodsPlan& p) {
  for (uint32_t chunks = 0; chunks <= p.chunks; chunks += (p.chunks > 16 && chunks > 4 && chunks + 5 < p.chunks ? 3 : 1)) {
    std::vector<int> owners(chunks, 0);
    uint32_t next = 0;
    for (uint32_t part = 0; part < p.split; ++part) {
      uint32_t c0 = 99, c1 = 99;
      periods_chunk_range(chunks, p.chunks, p.split, part, &c0, &c1);
      CHECK(c0 <= c1 && c1 <= chunks, "part %u of %u: [%u, %u) of %u", part, p.split, c0, c1, chunks);
      CHECK(c0 == next, "part %u starts at %u, not %u", part, c0, next);
      for (uint32_t c = c0; c < c1; ++c) ++owners[c];
      next = c1;
    }
    CHECK(next == chunks, "parts cover %u of %u chunks", next, chunks);
    for (uint32_t c = 0; c < chunks; ++c) CHECK(owners[c] == 1, "chunk %u has %d owners", c, owners[c]);
    ++checked_ranges;
  }
}

void check_plan(uint32_t span, uint32_t P, uint32_t cols, uint32_t L) {
  const uint32_t c = span / P;
  PeriodsPlan p;
  CHECK(periods_plan(P + 1, c, cols, L, 0, &p), "span %u P %u cols %u L %u", span, P, cols, L);
  CHECK(p.groups * kPeriodsSeriesGroup >= cols && (p.groups - 1) * kPeriodsSeriesGroup < cols, "groups %u of %u series", p.groups, cols);
  CHECK(p.blocks * kPeriodsLagBlock > L && (p.blocks - 1) * kPeriodsLagBlock <= L, "blocks %u of %u lags", p.blocks, L);
  CHECK(uint64_t(p.chunks) * kPeriodsChunk >= c && (p.chunks == 1 || uint64_t(p.chunks - 1) * kPeriodsChunk < c), "chunks %u of %u rows",
        p.chunks, c);
  CHECK(periods_pow2(p.split) && p.split <= p.chunks, "split %u of %u chunks", p.split, p.chunks);
  const uint64_t owned = uint64_t(P + 1) * p.groups * p.blocks;
  if (owned >= kPeriodsTargetGroups || p.chunks == 1) CHECK(p.split == 1, "owned: split %u", p.split);
  if (p.split > 1) CHECK(owned * (p.split / 2) < kPeriodsTargetGroups, "split %u is not the smallest", p.split);
  if (owned * p.split < kPeriodsTargetGroups) CHECK(p.split * 2 > p.chunks, "split %u could grow (chunks %u)", p.split, p.chunks);
  check_ranges(p);
  // every override the plan takes, and the ones it refuses
  for (uint32_t s = 1; s <= 2 * p.chunks && s <= 256; ++s) {
    PeriodsPlan q;
    const bool ok = periods_plan(P + 1, c, cols, L, s, &q);
    CHECK(ok == (periods_pow2(s) && s <= p.chunks), "override %u of %u chunks", s, p.chunks);
    if (!ok) continue;
    CHECK(q.split == s && q.groups == p.groups && q.blocks == p.blocks && q.chunks == p.chunks, "override %u", s);
    check_ranges(q);
  }
  ++checked_plans;
}

// the slots of [head - n, head) partition it in order, each inside one column
void check_slots(uint64_t head, uint32_t n, uint32_t c, uint32_t P) {
  uint64_t next = head - n, total = 0;
  for (uint32_t j = 0; j <= P; ++j) {
    uint64_t b = 99, e = 99;
    const bool full = periods_slot(head, n, c, P, j, &b, &e);
    if (!full) {
      CHECK(b == 0 && e == 0, "an empty slot is [0, 0)");
      continue;
    }
    CHECK(b < e && e - b <= c && b / c == (e - 1) / c, "slot %u: [%llu, %llu)", j, (unsigned long long)b, (unsigned long long)e);
    CHECK(b == next, "slot %u begins at %llu, not %llu", j, (unsigned long long)b, (unsigned long long)next);
    CHECK((e - 1) / c + P == (head - 1) / c + j, "slot %u is another column", j);
    next = e;
    total += e - b;
  }
  CHECK(total == n && (n == 0 || next == head), "slots hold %llu of %u rows", (unsigned long long)total, n);
  ++checked_slots;
}

}  // namespace

int main() {
  for (uint32_t span = 1u << 9; span <= 1u << 20; span <<= 1)
    for (uint32_t P = 8; P <= 64; P <<= 1) {
      const uint32_t c = span / P;
      if (c < 64 || c > 65536) continue;
      for (uint32_t cols : {1u, 5u, 8u, 9u, 12u, 16u, 61u, 64u})
        for (uint32_t L : {1u, 7u, 8u, 63u, 255u, 256u, 300u, 511u, 512u, 1023u, 1024u})
          if (2 * L <= c && P * (L + 1) <= 16384) check_plan(span, P, cols, L);
      for (int rep = 0; rep < 200; ++rep) {
        const uint64_t head = rep < 4 ? uint64_t(rep) * c : rnd() % (rep % 2 ? 1ull << 40 : 4ull * span);
        const uint32_t n = uint32_t(rnd() % (uint64_t(span) + 1));
        check_slots(head, uint32_t(n < head ? n : head), c, P);
        check_slots(head, uint32_t(span < head ? span : head), c, P);
      }
    }
  PeriodsPlan p;
  CHECK(periods_plan(17, 65536, 12, 255, 0, &p) && p.groups == 2 && p.blocks == 1 && p.chunks == 64, "2^20 rows in 16 columns");
  CHECK(p.split == 32, "34 owned items are split %u ways", p.split);
  CHECK(periods_plan(65, 1024, 12, 255, 0, &p) && p.split == 1 && p.chunks == 1, "the default shape is owned");
  std::printf("ok: %ld plans, %ld chunk ranges, %ld slot sets\n", checked_plans, checked_ranges, checked_slots);
  return 0;
}
