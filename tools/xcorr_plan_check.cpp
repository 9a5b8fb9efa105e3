// Host-only check of csrc/window_xcorr_plan.h, the text the cross-correlation kernel compiles:
// for every K from 1 to 8 random pairs (repeats and mirrored pairs included) are planned onto
// one, two or five rings of 2 to 64 series - every output slot must land in exactly one ring's
// list with the pair's own columns; for every K and a set of lag counts around the blocks of 256
// the whole grid (pair groups, lag blocks, threads, the 8 lags of a thread) is walked and every
// (pair, index of [2L + 1]) must be owned exactly once, every word a thread reads must lie
// within the rows its workgroup loaded and those within an LDS row; the chunks of a span must be
// shared among the workgroups exactly once; the refusals (K = 0, K = 9, a == b, an index beyond
// the set, a pair across rings, a ring wider than 64) must refuse. Build with
// -fsanitize=address,undefined and run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc tools/xcorr_plan_check.cpp -o check && ./check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "window_xcorr_plan.h"

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

long checked_plans = 0, checked_grids = 0, checked_shares = 0;

// rings of `stride` series each; K random pairs, each inside a random ring
void check_plan(uint32_t stride, uint32_t K, uint32_t nrings) {
  std::vector<XcorrRingSpan> spans;
  for (uint32_t r = 0; r < nrings; ++r) spans.push_back(XcorrRingSpan{r * stride, stride});
  std::vector<uint32_t> pairs;
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t r = rnd() % nrings, a = rnd() % stride;
    uint32_t b = rnd() % (stride - 1);
    if (b >= a) ++b;
    if (k > 0 && rnd() % 4 == 0) {  // a pair named twice, or its mirror
      const uint32_t j = rnd() % k, flip = rnd() % 2;
      pairs.push_back(pairs[2 * j + flip]);
      pairs.push_back(pairs[2 * j + 1 - flip]);
    } else {
      pairs.push_back(r * stride + a);
      pairs.push_back(r * stride + b);
    }
  }
  XcorrPlan plan;
  CHECK(xcorr_plan_pairs(pairs.data(), K, spans.data(), nrings, &plan), "stride %u K %u", stride, K);
  CHECK(plan.nrings >= 1 && plan.nrings <= K && plan.nrings <= nrings, "nrings %u", plan.nrings);
  uint32_t slot_seen = 0, last_ring = 0, total = 0;
  for (uint32_t i = 0; i < plan.nrings; ++i) {
    const XcorrRingPairs& p = plan.rings[i];
    CHECK(p.ring < nrings && (i == 0 || p.ring > last_ring), "ring order");
    last_ring = p.ring;
    CHECK(p.count >= 1 && p.count <= K, "count %u", p.count);
    total += p.count;
    for (uint32_t q = 0; q < p.count; ++q) {
      const uint32_t a = p.a[q], b = p.b[q], k = p.slot[q];
      CHECK(a < stride && b < stride && a != b, "columns %u %u", a, b);
      CHECK(k < K && !(slot_seen >> k & 1u), "slot %u twice", k);
      slot_seen |= 1u << k;
      CHECK(pairs[2 * k] == p.ring * stride + a && pairs[2 * k + 1] == p.ring * stride + b, "slot %u is another pair", k);
      CHECK(q == 0 || p.slot[q - 1] < k, "slots of a ring in order");
    }
  }
  CHECK(total == K && slot_seen == (1u << K) - 1u, "slots %x of K %u", slot_seen, K);
  ++checked_plans;
}

void check_refusals() {
  const XcorrRingSpan spans[2] = {{0, 11}, {11, 5}};
  XcorrPlan plan;
  const uint32_t ok[4] = {1, 2, 11, 12};
  CHECK(xcorr_plan_pairs(ok, 2, spans, 2, &plan) && plan.nrings == 2, "a pair in each ring");
  CHECK(xcorr_plan_pairs(ok, 1, spans, 2, &plan) && plan.nrings == 1 && plan.rings[0].ring == 0, "one ring without pairs");
  CHECK(xcorr_plan_pairs(ok + 2, 1, spans, 2, &plan) && plan.nrings == 1 && plan.rings[0].ring == 1 && plan.rings[0].a[0] == 0 &&
            plan.rings[0].b[0] == 1,
        "the second ring's columns");
  uint32_t nine[18];
  for (uint32_t i = 0; i < 9; ++i) nine[2 * i] = 0, nine[2 * i + 1] = 1 + i;
  CHECK(xcorr_plan_pairs(nine, 8, spans, 2, &plan), "eight pairs");
  CHECK(!xcorr_plan_pairs(nine, 9, spans, 2, &plan), "nine pairs");
  CHECK(!xcorr_plan_pairs(nine, 0, spans, 2, &plan), "no pair");
  CHECK(!xcorr_plan_pairs(nullptr, 1, spans, 2, &plan), "null pairs");
  const uint32_t same[2] = {3, 3}, beyond[2] = {0, 16}, across[2] = {10, 11}, across2[2] = {12, 2};
  CHECK(!xcorr_plan_pairs(same, 1, spans, 2, &plan), "a == b");
  CHECK(!xcorr_plan_pairs(beyond, 1, spans, 2, &plan), "beyond the set");
  CHECK(!xcorr_plan_pairs(across, 1, spans, 2, &plan), "across rings");
  CHECK(!xcorr_plan_pairs(across2, 1, spans, 2, &plan), "across rings, reversed");
  CHECK(!xcorr_plan_pairs(ok, 1, spans, 0, &plan), "no ring");
  const XcorrRingSpan wide[1] = {{0, 65}};
  CHECK(!xcorr_plan_pairs(ok, 1, wide, 1, &plan), "a ring wider than 64");
}

// the grid of `count` pairs and lags 0 .. L owns every (pair, index) exactly once and reads within its rows
void check_grid(uint32_t count, uint32_t L) {
  const uint32_t width = 2 * L + 1;
  std::vector<int> owners(size_t(count) * width, 0);
  const uint32_t groups = xcorr_pair_groups(count), blocks = xcorr_lag_blocks(L);
  CHECK(groups >= 1 && groups <= 2 && blocks >= 1 && blocks <= kMaxXcorrLags / kXcorrLagBlock + 1, "grid %u x %u", groups, blocks);
  uint32_t rows_total = 0;
  for (uint32_t g = 0; g < groups; ++g) {
    const uint32_t rows = xcorr_group_rows(count, g);
    CHECK(rows >= 2 && rows <= 2 * kXcorrGroupPairs && rows % 2 == 0, "rows %u", rows);
    rows_total += rows;
    for (uint32_t z = 0; z < blocks; ++z) {
      const uint32_t klo = z * kXcorrLagBlock, khi = xcorr_block_hi(L, z), tiles = xcorr_block_tiles(L, z);
      CHECK(klo <= khi && khi <= L && khi < klo + kXcorrLagBlock, "block %u: %u .. %u", z, klo, khi);
      CHECK(tiles >= 1 && rows * tiles <= kXcorrThreads, "tiles %u", tiles);
      const uint32_t len = xcorr_load_rows(khi);
      CHECK(len % 8 == 0 && len <= kXcorrPitch, "len %u", len);
      uint32_t threads = 0;
      for (uint32_t tid = 0; tid < kXcorrThreads; ++tid) {
        uint32_t r = 99, tile = 99;
        if (!xcorr_thread(tid, rows, tiles, &r, &tile)) {
          CHECK(r == 0 && tile == 0, "an idle thread points at row 0");
          continue;
        }
        ++threads;
        CHECK(r < rows && tile < tiles, "thread %u: item %u tile %u", tid, r, tile);
        const uint32_t k0 = klo + tile * kXcorrLagTile;
        // the walk reads y's words k0 .. k0 + chunk + 7 and the prefix path its blocks up to k0 + chunk
        CHECK(k0 % 8 == 0 && k0 <= khi && k0 + kXcorrChunk + 8 <= len, "thread %u reads to %u of %u", tid, k0 + kXcorrChunk + 8, len);
        const uint32_t pair = g * kXcorrGroupPairs + (r >> 1);
        CHECK(pair < count, "pair %u", pair);
        for (uint32_t j = 0; j < kXcorrLagTile; ++j) {
          const int32_t idx = xcorr_index(L, r, k0 + j);
          CHECK(idx >= -1 && idx < int32_t(width), "index %d", idx);
          if (idx < 0) continue;
          CHECK((r & 1u) ? uint32_t(idx) == L - (k0 + j) && k0 + j >= 1 : uint32_t(idx) == L + k0 + j, "index %d of lag %u", idx, k0 + j);
          ++owners[size_t(pair) * width + uint32_t(idx)];
        }
      }
      CHECK(threads == rows * tiles, "threads %u", threads);
    }
  }
  CHECK(rows_total == 2 * count, "rows %u of %u pairs", rows_total, count);
  for (size_t i = 0; i < owners.size(); ++i)
    CHECK(owners[i] == 1, "pair %zu index %zu has %d owners (L %u)", i / width, i % width, owners[i], L);
  ++checked_grids;
}

// the chunks of a span are shared among the workgroups exactly once
void check_shares(uint32_t chunks, uint32_t per_chunk) {
  const uint32_t share = xcorr_share(chunks, per_chunk), groups = xcorr_share_groups(chunks, share);
  CHECK(share >= 1 && groups >= 1 && groups <= chunks, "share %u groups %u", share, groups);
  CHECK(groups == 1 || groups <= kXcorrTargetGroups / per_chunk, "%u workgroups", groups * per_chunk);
  uint32_t next = 0;
  for (uint32_t g = 0; g < groups; ++g) {
    const uint32_t c0 = g * share, c1 = (g + 1) * share < chunks ? (g + 1) * share : chunks;
    CHECK(c0 == next && c0 < c1, "share of group %u starts at %u, not %u", g, c0, next);
    next = c1;
  }
  CHECK(next == chunks, "shares cover %u of %u chunks", next, chunks);
  ++checked_shares;
}

}  // namespace

int main() {
  for (uint32_t stride = 2; stride <= 64; ++stride)
    for (uint32_t K = 1; K <= kMaxXcorrPairs; ++K)
      for (uint32_t nrings : {1u, 2u, 5u})
        for (int rep = 0; rep < 8; ++rep) check_plan(stride, K, nrings);
  check_refusals();
  for (uint32_t count = 1; count <= kMaxXcorrPairs; ++count)
    for (uint32_t L : {1u, 2u, 7u, 8u, 9u, 63u, 64u, 70u, 200u, 247u, 248u, 255u, 256u, 257u, 300u, 511u, 512u, 767u, 1023u, 1024u})
      check_grid(count, L);
  for (uint32_t chunks = 1; chunks <= 1100; chunks += (chunks < 70 ? 1 : 1 + rnd() % 13))
    for (uint32_t per_chunk = 1; per_chunk <= 10; ++per_chunk) check_shares(chunks, per_chunk);
  check_shares(1024, 1);
  check_shares(1024, 10);
  std::printf("ok: %ld plans, %ld grids, %ld shares\n", checked_plans, checked_grids, checked_shares);
  return 0;
}
