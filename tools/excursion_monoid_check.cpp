// Host-only check of csrc/window_excursions_monoid.h, the text the kernels compile: random
// sample sequences (valid / invalid, above / not) are cut into random pieces - empty ones
// included - each piece is folded with excursion_push, the pieces are combined in order with
// excursion_combine under a random bracketing, and the record is compared with a plain loop
// over the samples. Build with -fsanitize=address,undefined and run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc tools/excursion_monoid_check.cpp -o check && ./check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "window_excursions_monoid.h"

using rocmdash::ExcursionPartial;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return uint32_t((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Sample {
  bool valid, above;
};

void loop_record(const std::vector<Sample>& x, int32_t out[8]) {
  int32_t above = 0, valid = 0, episodes = 0, longest = 0, run = 0, since = 0, leading = -1;
  for (const Sample& s : x) {
    if (!s.valid) continue;
    ++valid;
    if (s.above) {
      ++above;
      if (++run == 1) ++episodes;
      if (run > longest) longest = run;
      since = 0;
    } else {
      if (leading < 0) leading = run;
      run = 0;
      ++since;
    }
  }
  if (leading < 0) leading = run;
  const int32_t r[8] = {above, valid, episodes, longest, run, since, leading, int32_t(x.size())};
  for (int i = 0; i < 8; ++i) out[i] = r[i];
}

// the pieces [lo, hi) combined in order, split at a random point: every bracketing occurs
ExcursionPartial fold(const std::vector<ExcursionPartial>& p, size_t lo, size_t hi) {
  if (hi == lo) return ExcursionPartial{0, 0, 0, 0, 0, 0, 0};
  if (hi - lo == 1) return p[lo];
  const size_t mid = lo + 1 + rnd() % (hi - lo - 1);
  return rocmdash::excursion_combine(fold(p, lo, mid), fold(p, mid, hi));
}

}  // namespace

int main() {
  int bad = 0;
  for (int trial = 0; trial < 4000 && bad < 5; ++trial) {
    const size_t n = rnd() % 200;
    const uint32_t p_above = rnd() % 101, p_nan = trial % 3 == 0 ? 0 : rnd() % 40, mean_run = 1 + rnd() % 20;
    std::vector<Sample> x(n);
    bool up = rnd() & 1;
    for (Sample& s : x) {
      if (rnd() % mean_run == 0) up = rnd() % 100 < p_above;
      s = Sample{rnd() % 100 >= p_nan, up};
    }
    std::vector<size_t> cuts{0};
    while (cuts.back() < n) cuts.push_back(cuts.back() + rnd() % (n - cuts.back() + 1));  // empty pieces too
    cuts.push_back(n);
    std::vector<ExcursionPartial> parts;
    for (size_t i = 0; i + 1 < cuts.size(); ++i) {
      ExcursionPartial p{0, 0, 0, 0, 0, 0, 0};
      for (size_t j = cuts[i]; j < cuts[i + 1]; ++j) rocmdash::excursion_push(p, x[j].valid, x[j].above);
      parts.push_back(p);
    }
    int32_t got[8], want[8];
    rocmdash::excursion_record(fold(parts, 0, parts.size()), uint32_t(n), got);
    loop_record(x, want);
    for (int i = 0; i < 8; ++i)
      if (got[i] != want[i]) {
        std::printf("trial %d (n = %zu, %zu pieces): field %d is %d, the loop says %d\n", trial, n, parts.size(), i, got[i],
                    want[i]);
        ++bad;
        break;
      }
  }
  std::printf(bad ? "FAILED\n" : "ok: 4000 random sequences\n");
  return bad ? 1 : 0;
}
