// Host-only check of csrc/window_joint_plan.h, the text the joint-histogram kernel compiles:
// for every ring stride from 2 to 64 and every K from 1 to 8 random pairs (repeats included)
// are planned onto one, two or five rings - so that rings have none, one or several pairs -
// and every distinct pair must have exactly one owner (lane of the row, pass) per row, every
// output slot exactly one distinct pair, and the packed columns must be the pair's; windows,
// wrapped and not, must be cut into blocks that cover their rows exactly once, and the pieces
// of a block must be shared among the workgroups exactly once, in whole rows; the refusals
// (K = 0, K = 9, a == b, an index beyond the set, a pair across rings) must refuse. Build with
// -fsanitize=address,undefined and run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc tools/joint_plan_check.cpp -o check && ./check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "window_joint_plan.h"

using namespace rocmdash;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return uint32_t((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
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

long checked_plans = 0, checked_cuts = 0, checked_shares = 0;

// rings of `stride` series each; K random pairs, each inside a random ring
void check_plan(uint32_t stride, uint32_t K, uint32_t nrings) {
  std::vector<JointRingSpan> spans;
  for (uint32_t r = 0; r < nrings; ++r) spans.push_back(JointRingSpan{r * stride, stride});
  std::vector<uint32_t> pairs;
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t r = rnd() % nrings, a = rnd() % stride;
    uint32_t b = rnd() % (stride - 1);
    if (b >= a) ++b;
    if (k > 0 && rnd() % 4 == 0) {  // a pair named twice
      const uint32_t j = rnd() % k;
      pairs.push_back(pairs[2 * j]);
      pairs.push_back(pairs[2 * j + 1]);
    } else {
      pairs.push_back(r * stride + a);
      pairs.push_back(r * stride + b);
    }
  }
  JointPlan plan;
  CHECK(joint_plan_pairs(pairs.data(), K, spans.data(), nrings, &plan), "stride %u K %u", stride, K);
  CHECK(plan.nrings >= 1 && plan.nrings <= K && plan.nrings <= nrings, "nrings %u", plan.nrings);
  uint32_t slot_seen = 0, last_ring = 0;
  for (uint32_t i = 0; i < plan.nrings; ++i) {
    const JointRingPairs& p = plan.rings[i];
    CHECK(p.ring < nrings && (i == 0 || p.ring > last_ring), "ring order");
    last_ring = p.ring;
    CHECK(p.distinct >= 1 && p.distinct <= K && p.distinct <= kJointOwnerPasses * stride, "distinct %u stride %u",
          p.distinct, stride);
    // exactly one owner (lane of the row, pass) per distinct pair, none beyond them
    std::vector<int> owners(p.distinct, 0);
    for (uint32_t pass = 0; pass < kJointOwnerPasses + 1; ++pass)
      for (uint32_t c = 0; c < stride + 2; ++c) {
        const int q = joint_owned_pair(stride, p.distinct, c, pass);
        CHECK(q >= -1 && q < int(p.distinct), "q %d", q);
        if (q >= 0) {
          CHECK(c < stride && pass < kJointOwnerPasses, "owner outside the row");
          ++owners[q];
        }
      }
    for (uint32_t q = 0; q < p.distinct; ++q) {
      CHECK(owners[q] == 1, "pair %u of ring %u has %d owners (stride %u)", q, p.ring, owners[q], stride);
      const uint32_t a = joint_byte(p.a, q), b = joint_byte(p.b, q), m = joint_byte(p.slots, q);
      CHECK(a < stride && b < stride && a != b && m != 0, "columns %u %u slots %u", a, b, m);
      for (uint32_t k = 0; k < kMaxJointPairs; ++k) {
        if (!(m >> k & 1u)) continue;
        CHECK(k < K && !(slot_seen >> k & 1u), "slot %u twice", k);
        slot_seen |= 1u << k;
        CHECK(pairs[2 * k] == p.ring * stride + a && pairs[2 * k + 1] == p.ring * stride + b, "slot %u is another pair", k);
      }
      for (uint32_t o = 0; o < q; ++o)
        CHECK(!(joint_byte(p.a, o) == a && joint_byte(p.b, o) == b), "pair %u repeats %u", q, o);
    }
    for (uint32_t q = p.distinct; q < kMaxJointPairs; ++q)
      CHECK(joint_byte(p.a, q) == 0 && joint_byte(p.b, q) == 0 && joint_byte(p.slots, q) == 0, "bytes beyond the pairs");
  }
  CHECK(slot_seen == (1u << K) - 1u, "slots %x of K %u", slot_seen, K);
  ++checked_plans;
}

void check_refusals() {
  const JointRingSpan spans[2] = {{0, 11}, {11, 5}};
  JointPlan plan;
  const uint32_t ok[4] = {1, 2, 11, 12};
  CHECK(joint_plan_pairs(ok, 2, spans, 2, &plan) && plan.nrings == 2, "a pair in each ring");
  CHECK(joint_plan_pairs(ok, 1, spans, 2, &plan) && plan.nrings == 1 && plan.rings[0].ring == 0, "one ring without pairs");
  CHECK(joint_plan_pairs(ok + 2, 1, spans, 2, &plan) && plan.nrings == 1 && plan.rings[0].ring == 1 &&
            joint_byte(plan.rings[0].a, 0) == 0 && joint_byte(plan.rings[0].b, 0) == 1,
        "the second ring's columns");
  uint32_t nine[18];
  for (uint32_t i = 0; i < 9; ++i) nine[2 * i] = 0, nine[2 * i + 1] = 1 + i;
  CHECK(joint_plan_pairs(nine, 8, spans, 2, &plan), "eight pairs");
  CHECK(!joint_plan_pairs(nine, 9, spans, 2, &plan), "nine pairs");
  CHECK(!joint_plan_pairs(nine, 0, spans, 2, &plan), "no pair");
  CHECK(!joint_plan_pairs(nullptr, 1, spans, 2, &plan), "null pairs");
  const uint32_t same[2] = {3, 3}, beyond[2] = {0, 16}, across[2] = {10, 11}, across2[2] = {12, 2};
  CHECK(!joint_plan_pairs(same, 1, spans, 2, &plan), "a == b");
  CHECK(!joint_plan_pairs(beyond, 1, spans, 2, &plan), "beyond the set");
  CHECK(!joint_plan_pairs(across, 1, spans, 2, &plan), "across rings");
  CHECK(!joint_plan_pairs(across2, 1, spans, 2, &plan), "across rings, reversed");
  CHECK(!joint_plan_pairs(ok, 1, spans, 0, &plan), "no ring");
  const JointRingSpan wide[1] = {{0, 65}};
  CHECK(!joint_plan_pairs(ok, 1, wide, 1, &plan), "a ring wider than a wave");
}

// the blocks of a window cover its rows exactly once
void check_cut(uint64_t depth, uint64_t head, uint64_t rows) {
  const JointCut c = joint_cut(depth, head, rows);
  std::vector<uint8_t> seen(depth, 0);
  CHECK(c.tail + c.rest == rows && c.first + c.tail <= depth && c.rest <= c.first, "cut %llu %llu %llu",
        (unsigned long long)depth, (unsigned long long)head, (unsigned long long)rows);
  for (uint64_t i = 0; i < c.tail; ++i) ++seen[c.first + i];
  for (uint64_t i = 0; i < c.rest; ++i) ++seen[i];
  std::vector<uint8_t> want(depth, 0);
  for (uint64_t r = head - rows; r < head; ++r) ++want[r & (depth - 1)];
  CHECK(seen == want, "blocks of depth %llu head %llu rows %llu", (unsigned long long)depth, (unsigned long long)head,
        (unsigned long long)rows);
  // time order: block 0 starts at the window's oldest row
  if (rows) CHECK(c.first == ((head - rows) & (depth - 1)), "first");
  ++checked_cuts;
}

// the pieces of a block are whole rows and are shared among the workgroups exactly once
void check_shares(uint32_t stride, uint64_t rows, uint32_t groups) {
  const uint64_t F = rows * stride;
  const uint32_t L = joint_piece_floats(stride), pieces = joint_pieces(F, stride), share = joint_share(pieces, groups);
  CHECK(L % stride == 0 && L >= stride && L <= 64 && L + stride > 64, "L %u stride %u", L, stride);
  CHECK(uint64_t(pieces) * L >= F && uint64_t(pieces - 1) * L < F, "pieces %u", pieces);
  uint64_t floats = 0;
  uint32_t next = 0;
  for (uint32_t g = 0; g < groups; ++g) {
    const uint32_t pb = g * share;
    if (pb >= pieces) continue;
    const uint32_t pe = pb + share < pieces ? pb + share : pieces;
    CHECK(pb == next, "share of group %u starts at %u, not %u", g, pb, next);
    next = pe;
    for (uint32_t k = pb; k < pe; ++k) {
      const uint64_t i0 = uint64_t(k) * L, have = F - i0 < L ? F - i0 : L;
      CHECK(i0 < F && have % stride == 0 && have > 0, "piece %u", k);
      floats += have;
    }
  }
  CHECK(next == pieces && floats == F, "shares cover %llu of %llu floats", (unsigned long long)floats, (unsigned long long)F);
  ++checked_shares;
}

}  // namespace

int main() {
  for (uint32_t stride = 2; stride <= 64; ++stride)
    for (uint32_t K = 1; K <= kMaxJointPairs; ++K)
      for (uint32_t nrings : {1u, 2u, 5u})
        for (int rep = 0; rep < 8; ++rep) check_plan(stride, K, nrings);
  check_refusals();
  for (uint64_t depth : {1ull, 2ull, 8ull, 64ull, 256ull})
    for (uint64_t rows = 0; rows <= depth; rows += (depth > 16 ? 1 + rnd() % 7 : 1))
      for (uint64_t head = rows; head <= rows + 3 * depth; head += (depth > 16 ? 1 + rnd() % 5 : 1)) check_cut(depth, head, rows);
  for (uint32_t stride = 1; stride <= 64; ++stride)
    for (uint64_t rows : {1ull, 2ull, 63ull, 64ull, 65ull, 4096ull, 100003ull})
      for (uint32_t groups : {1u, 2u, 7u, 768u}) check_shares(stride, rows, groups);
  std::printf("ok: %ld plans, %ld cuts, %ld shares\n", checked_plans, checked_cuts, checked_shares);
  return 0;
}
