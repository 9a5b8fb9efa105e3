// The long-window kernels' argument blocks and what they point at: constants, the
// device-visible records and the host launchers. Shared by the kernel files and the host
// class (long_window.hip); holds no device code.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "long_window.h"

namespace rocmdash {

constexpr int NT = 256;
constexpr int kSlots = 16;  // pinned parameter staging slots
constexpr int kD0 = 10;                 // pass 0 digit: at most 10 key bits, 1024 bins
constexpr uint32_t kB0 = 1u << kD0;
constexpr uint32_t kPredMaxNew = NT;    // new rows pass 0 reads for its prediction (one per thread)

struct LwParams {
  uint64_t head[kLongMaxRings];
  uint64_t prev_head[kLongMaxRings];  // the head at this set's previous refresh (0: none)
  uint32_t n[kLongMaxRings];
  float pct[3];
  uint32_t seq;  // this refresh's number: the host-mapped report word carries it
};

struct LwPartial {  // one (series, chunk): identity = {0, 0, ~0u, 0, 0, 0}
  double sum;
  uint32_t cnt, minkey, maxkey, orx;  // orx: OR of (key ^ ref) - the bits that vary
  // the key orx is relative to: a window member while cnt > 0 (the newest sample when the
  // chunk was streamed: a chunk is streamed again before W rows entered). Partials of
  // different refreshes combine exactly in the lowest varying bit: orx_a | orx_b | (ref_a
  // ^ ref_b) (lw_combine) - the only bit of orx anything reads
  uint32_t ref, pad;
};

// Node mode (refresh_node): one series' predicted key range on one rank, all-gathered so
// that every rank histograms the SAME digit in pass 0.
struct LwPred {
  uint32_t pmin, pmax;  // predicted key range (0 / ~0: no prediction)
  uint32_t lo;          // lowest key bit predicted to vary
  uint32_t ref;         // key of the ring's newest sample (a window member when has)
  uint32_t has;         // the ring holds samples
  uint32_t pad[3];
};

struct LwSel {  // one series, carried from scan to scan (min / max also to the next refresh)
  uint32_t nv, minkey, maxkey;
  uint32_t done;   // bracket mode: scan B resolved the series this refresh (the radix chain skips it)
  double sum;
  uint32_t shift;  // prefix bits >= shift are found
  uint32_t width;  // the next digit: key bits [shift - width, shift); 0 = resolved
  uint32_t lo;     // lowest bit that varies over the window (32: none)
  uint32_t pad2;
  uint32_t resid[kLongRanks];   // rank inside the bucket the prefix names
  uint32_t prefix[kLongRanks];  // key bits found so far (high bits first)
};

// Bracket mode (long_window_brackets.hip): one bracket per percentile around the previous
// refresh's percentile keys.
constexpr int kPassBrk = 4;
constexpr int kBrkQ = 3;                  // one bracket per percentile (its lo and hi position)
constexpr uint32_t kBrkTarget = 2048;     // samples a bracket aims to hold
constexpr uint32_t kBrkCap = 8192;        // kept keys scan B selects among (LDS)
constexpr uint32_t kSelBits = 8;          // scan B's LDS radix digit (one bin per thread: no bank conflicts, one-word scans)
struct LwBrk {  // one series (persists across refreshes)
  uint32_t lo[kBrkQ], hi[kBrkQ];  // key bounds, inclusive (lo <= hi)
  uint32_t delta[kBrkQ];          // half-width in VALUE units (float bits; 0: an exact-key bracket)
  uint32_t cin[kBrkQ];            // samples inside at the last refresh that used it
  uint32_t valid;                 // the bounds apply to the next refresh
  uint32_t hit;                   // the last refresh was resolved by the brackets
  uint32_t refreshes, hits;       // counters (diagnostics)
  uint32_t nounion[kBrkQ];        // the last miss overflowed: the next exact bracket is only the new keys
  uint32_t dsave[kBrkQ];          // the value half-width an overflow put aside (float bits; 0: none)
};
struct LwBrkPart {  // one (series, chunk) of pass B
  uint32_t lt[kBrkQ];   // samples below the bracket
  uint32_t mid[kBrkQ];  // samples strictly inside (lo < k < hi): the kept keys of the slab
  uint32_t eq[kBrkQ];   // samples ON the bounds: count(k == lo) | count(k == hi, hi != lo) << 16
};                      // (a chunk holds < 2^16 rows); they are counted, never kept

// Node bracket mode (refresh_node): the node's brackets aim at fewer samples (the union of
// the ranks' kept keys crosses the node), and every rank contributes at most `cap` keys per
// bracket (<= kNodeCap); more (or a chunk slab that overflowed) is a miss and the node
// radix chain resolves the series. kNodeBrkRanks: the most ranks whose union fits scan B's
// LDS.
constexpr uint32_t kNodeBrkTarget = 256;  // 2x it (a sized bracket's most) fits one rank's kNodeCap twice over
constexpr uint32_t kNodeCap = 1024;
constexpr uint32_t kNodeBrkRanks = 8;
struct LwNodeHdr {  // one rank, one series (all-gathered over the node)
  LwPartial p;                      // the rank's partials over its chunks
  uint32_t lt[kBrkQ], mid[kBrkQ];   // below / strictly inside each node bracket
  uint32_t elo[kBrkQ], ehi[kBrkQ];  // on its lower / upper bound (counted, not kept)
  uint32_t ovf;                     // bracket bits whose kept keys did not all fit
  uint32_t ent;                     // rows that entered the rank's window since its last refresh (~0: unknown)
  uint32_t pad[2];
};
static_assert(sizeof(LwNodeHdr) % sizeof(LwPartial) == 0, "records stride in partials");
// One rank's all-gathered block: the S headers, then the kept keys [S][kBrkQ][cap] (chunk
// order). `cap` is the refresh's record cap, the same on every rank (LongWindowSet::
// node_cap_: sized from the previous refresh's node-wide most kept keys), so the one
// collective carries ~2x the keys the node's brackets keep, not kNodeCap per bracket: at
// 8 ranks 12 series move 20 KB per rank instead of 150 KB.
__host__ __device__ constexpr size_t lw_node_block(uint32_t S, uint32_t cap) {
  return size_t(S) * (sizeof(LwNodeHdr) + kBrkQ * sizeof(uint32_t) * size_t(cap));
}
// the next refresh's record cap from this one's most kept keys of any (rank, series,
// bracket) that a cap could hold (<= kNodeCap; a bracket over it re-sizes): 2x headroom, a floor of 4x a rank's share of the node target, 64-key steps
// (keeps every block a multiple of the partials' 32 B), at most kNodeCap
inline uint32_t lw_node_cap_next(uint32_t maxmid, uint32_t nranks) {
  uint32_t c = 2 * maxmid;
  const uint32_t floor = 4 * kNodeBrkTarget / (nranks ? nranks : 1);
  if (c < floor) c = floor;
  c = (c + 63) / 64 * 64;
  return c < kNodeCap ? c : kNodeCap;
}

// pass B keeps at most this many keys per (chunk, bracket): a bracket holds ~kBrkTarget of
// the window's samples, so a chunk is rarely near it; a fuller chunk makes scan B miss
// (the radix chain resolves the series, exact) and the bracket narrows. 3 / 64 of the
// window per series of HBM (the slabs were 3 / 4 of it, plus compaction's)
__host__ __device__ constexpr uint32_t lw_qcap(uint32_t chunk_rows) {
  return chunk_rows / 64 > 64 ? chunk_rows / 64 : 64;
}

struct LwRing {
  const float* dev;
  uint32_t width, first_series;
  uint32_t chunk_rows;  // rows one pass workgroup streams (per ring: balanced by row bytes)
  uint32_t nchunks;     // workgroups per segment of the ring
  uint32_t qcap;        // pass B: kept keys per (chunk, bracket) slab (lw_qcap)
  uint32_t pad;
  uint64_t boff;        // pass B slabs: the ring's first series' keys in LwArgs::bcand
  uint64_t bstride;     // keys per series: nchunks x kBrkQ x qcap
};

// A pass workgroup streams the rows of one ring segment: <= 8 of its series (a 16-wide
// ring is two segments), so no code path holds more than 8 series' state in registers.
// The pass grid is flat: segment g owns workgroups [wg0, wg0 + its ring's nchunks).
constexpr uint32_t kSegCols = 8;
struct LwSeg {
  uint32_t ring, col0, ncols, wg0;
};

struct LwArgs {
  // ---- the radix chain (every refresh that runs it) ----
  LwRing rings[kLongMaxRings];
  LwSeg segs[2 * kLongMaxRings];
  uint32_t num_rings, num_segs, num_series, mask, max_chunks;  // max_chunks: over the rings
  const LwParams* params;
  LwPartial* part;  // [S][max_chunks]; slots past a ring's nchunks hold the identity
  uint32_t* hist0;  // [S][kB0]
  uint32_t* histk;  // [S][6][256]
  LwSel* sel;       // [S]
  uint32_t* dig0;   // [S][3]: pass 0's digit shift, the reference key of its orx, digit width
  float* out;       // [S][8]
  // ---- the node chain (0 = this rank's window only): ranks whose windows form the node window ----
  uint32_t node_n;
  LwPred* pred_local;       // [S] this rank's prediction
  const LwPred* pred_all;   // [node_n][S] every rank's (all-gathered)
  LwPartial* agg_local;     // [S] this rank's partials reduced over its chunks
  const LwPartial* agg_all; // [node_n][S] every rank's (all-gathered)
  uint32_t wave_priv;       // (chain) pass 0: per-wave LDS histogram copies for 8-bit digits
  // ---- brackets (0: off - disabled, or no series wants them): pass B + scan B run first, and
  // the radix chain skips the series scan B resolved (LwSel::done) ----
  uint32_t brk_on;
  LwBrk* brk;               // [S] the next refresh's brackets
  LwBrk* brk_used;          // [S] the brackets this refresh's pass B used (its copy)
  uint32_t* hflags;         // [S] host-mapped: a series wants brackets (a launch hint; may be null)
  LwBrkPart* bpart;         // [S][max_chunks]
  uint32_t* bcand;          // pass B's kept keys (LwRing::boff / bstride / qcap)
  // ---- incremental and fused brackets (incr): a bracket stays put while the percentiles sit
  // well inside it, so the chunks' counts stay valid and pass B streams only the chunks new
  // rows landed in (its grid: the work list, seg << 20 | chunk; nwork = 0: every chunk).
  // colsplit: the list is seg << 23 | column << 20 | chunk - one workgroup per (chunk,
  // series): a short list's few chunks then spread over 8x the CUs (a lone workgroup
  // streaming a whole chunk of 8 series is latency-bound), with the same sums ----
  uint32_t incr;
  const uint32_t* work;
  uint32_t nwork;
  uint32_t colsplit;
  uint32_t* bchg;           // [S] host-mapped: the series' brackets changed (its chunks' counts are stale)
  const uint32_t* fwork;    // lw_scan_brk_fused: the chunks scan B streams itself (seg << 20 | chunk)
  uint32_t nfused;
  unsigned long long* report;  // host-mapped: seq (24 bits) | series the chain must resolve (24) | node select's most
                               // kept keys of one rank's bracket (16) - lw_brk_finish: one 8-byte system-scope store
  // ---- node brackets ----
  uint32_t node_brk;        // the brackets are the node's (refresh_node): their target is kNodeBrkTarget
  unsigned char* nbl;       // this rank's node-bracket block (lw_node_block(S, node_cap) bytes)
  // ---- diagnostics ----
  unsigned long long* dbg;  // (null: off) scan B's phase clocks [S][kBrkQ][8]
  // ---- brackets, again (the layout is fixed: kernels and the host share it) ----
  uint32_t* brk_cnt;        // device [2]: scan B's finished workgroups (the last one writes the report);
                            // node select's most kept keys of one rank's bracket (the report's top 16 bits)
  uint32_t brk_target;      // samples a local bracket aims to hold (LongWindowSet::brk_target, <= kBrkTarget)
  // ---- node brackets, again ----
  const unsigned char* nball;  // [node_n] every rank's block (all-gathered)
  uint32_t node_cap;        // the records' key cap (a multiple of 64, <= kNodeCap)

  // ---- candidate compaction (compact = 0: off): pass 2 keeps the keys of the samples it counts
  // (those whose found bits match a rank's prefix) and pass 3 histograms those instead of
  // streaming the window again. Workgroup c of pass 2 owns the slab
  // cand[s][c * chunk_rows ..) of each of its series (its chunk has that many rows, so the
  // slab never overflows) and counts into it with LDS atomics: no device atomics. ----
  uint32_t compact;
  uint32_t* cand;           // [S][cand_cap]: compaction's slabs (pass B's are bcand)
  uint32_t* cand_n;         // [S][max_chunks] keys in each slab
  uint32_t cand_cap;        // >= nchunks x chunk_rows of every ring (>= W)
};
static_assert(sizeof(LwArgs) == 624, "the kernels' argument block: layout and size are fixed");

// lw_ingest (long_window_brackets.hip): a small refresh's staging in one launch.
struct LwIngestSeg {
  const float* src;  // host ring rows (device view)
  float* dst;        // device window rows
  uint32_t floats;
  uint32_t pad;
};
constexpr int kIngestSegs = 2 * kLongMaxRings;
struct LwIngest {
  const LwParams* hp;  // the slot (device view)
  LwParams* dp;
  const uint32_t* hwork;
  uint32_t* dwork;
  uint32_t nwork;
  uint32_t nseg;
  LwIngestSeg seg[kIngestSegs];
  const uint32_t* bsrc;  // the fused pass B's brackets: brk -> brk_used (bwords = 0: none), its own workgroup
  uint32_t* bdst;
  uint32_t bwords;
};

// ---- host launchers: each kernel is defined in exactly one .hip file and reached from the
// others only through these (no relocatable device code). Grids a launcher does not take
// follow from the arguments: one workgroup per series, per (series, bracket), or per segment.
// long_window_radix.hip
void lw_launch_node_predict(hipStream_t stream, const LwArgs& a);
void lw_launch_node_partials(hipStream_t stream, const LwArgs& a);
// pass 0..3 over `grid` workgroups; prefetch: LongWindowSet::set_prefetch's mode
void lw_launch_pass(int pass, int prefetch, uint32_t grid, size_t lds, hipStream_t stream, const LwArgs& a);
void lw_launch_pass_cand(hipStream_t stream, const LwArgs& a);  // pass 3 over pass 2's candidates
void lw_launch_scan(int pass, hipStream_t stream, const LwArgs& a);
// long_window_brackets.hip
void lw_launch_pass_brk(uint32_t grid, hipStream_t stream, const LwArgs& a);
void lw_launch_scan_brk(bool fused, hipStream_t stream, const LwArgs& a);  // + the report
void lw_launch_node_brk_local(hipStream_t stream, const LwArgs& a);
void lw_launch_node_brk_select(hipStream_t stream, const LwArgs& a);  // + the report
void lw_launch_ingest(hipStream_t stream, const LwIngest& in);

}  // namespace rocmdash
