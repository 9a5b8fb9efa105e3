// Window excursions: per series and threshold, the episodes a window spent above the
// threshold - how many, the longest, the current one, the samples since the last - the one
// view of a window in which the ORDER of the samples is the result (window_stats.h,
// window_buckets.h and window_trend.h are order-free reductions). The semantics are stated
// once, in rocmdash/ops/window_excursions.py; in short: NaN samples are skipped and all
// lengths count valid samples, x > t (strictly) is above, an episode is a maximal run of
// above samples among the valid ones.
//
// Per (series, threshold) one record of eight int32 (two 16-byte stores):
//   {above, valid, episodes, longest, current, since, leading, rows}.
//
// One pass over the time-major device ring. The window is one contiguous block of rows, or
// two when it wraps, the older first; each block is cut into chunks of consecutive rows, a
// workgroup takes one (chunk, ring), each of its waves a contiguous quarter of the chunk and
// each lane a contiguous run of rows of one series, which it folds sample by sample into
// the monoid of window_excursions_monoid.h, in registers. Lanes of one series combine in
// time order through shuffles, the waves in wave order through LDS, and the workgroup
// stores one partial per (chunk, series, threshold) into the caller's workspace. A second,
// small kernel combines a ring's partials in chunk order and writes the records. No
// atomics and no tickets: the order of combination is the result, and any chunking of the
// same window gives the same bits.
//
// Three entries over the one device routine:
//   * launch_excursion_ring: one ring of series described by value;
//   * DeviceWindowSet::export_excursions (device_window.h): the device rings of the last refresh;
//   * LongWindowSet::export_excursions (long_window.h): the long windows of the last refresh.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rocmdash {

constexpr uint32_t kMaxExcursionThresholds = 4;
constexpr uint32_t kMaxExcursionStride = 64;     // floats per ring row: a wave holds at least one row
constexpr uint32_t kMaxExcursionChunks = 1024;   // per ring: 4 workgroups of 4 waves per CU, all resident
constexpr uint32_t kMinExcursionChunkRows = 256; // a planned chunk: >= 64 rows per wave
constexpr uint32_t kExcursionFields = 8;
constexpr int kExcursionRingsPerLaunch = 8;

// Bytes of workspace for `series` series (one ring's stride, or every series of a set) and
// K thresholds: kMaxExcursionChunks partials of 32 bytes per (series, threshold). 0 for a K
// outside [1, 4]. The workspace is the caller's, 16-byte aligned; nothing in it needs to be
// initialised and nothing of it is read that the same call did not write.
size_t excursion_workspace_bytes(uint32_t series, uint32_t K);

// Rows per chunk as planned for a window of n rows: the smallest that keeps a window cut in
// two blocks within kMaxExcursionChunks chunks, at least kMinExcursionChunkRows.
uint32_t excursion_plan_chunk_rows(uint32_t n);

// Chunks of the window [head - n, head) of a ring of `depth` rows cut every chunk_rows rows
// (each of its one or two blocks on its own).
uint64_t excursion_chunk_count(uint32_t depth, uint64_t head, uint32_t n, uint32_t chunk_rows);

// base: device ring [depth][stride] floats, row r at slot r & (depth - 1), of which the first
// `cols` columns are series; the window is rows [head - n, head). thresholds: device
// [cols][K] floats, finite and strictly increasing per series. chunk_rows: 0 plans the
// chunks; otherwise that many rows per chunk. dst: device [cols][K][8] int32, 16-byte
// aligned. work: device, 16-byte aligned, work_bytes >= excursion_workspace_bytes(stride, K).
// n == 0: all-zero records. Returns a hipError_t: hipErrorInvalidValue, before any launch or
// write, unless depth is a power of two, n <= depth, n <= head, 1 <= cols <= stride <= 64,
// 1 <= K <= 4, the chunks number at most kMaxExcursionChunks, the workspace is large enough
// and every pointer is set and aligned (base and thresholds to 4 bytes).
int launch_excursion_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                          const float* thresholds, uint32_t K, uint32_t chunk_rows, int32_t* dst, void* work,
                          size_t work_bytes, void* stream);

}  // namespace rocmdash
