// Window autocorrelation: exact integer lag sums of every series of a ring - the rhythm of a
// series (its period, and how strong it is), which no per-level export can tell. The semantics
// are stated once, in rocmdash/ops/window_autocorr.py: over the newest N = min(n, span) rows
// of the window, a sample is quantised to q in [0, 4095] by one fp32 multiply with scale[s] and
// a round half to even (NaN: invalid, v = 0 and q = 0), and for every lag k = 0 .. L the output
// holds the four sums over 0 <= t < N - k of v[t] v[t+k], q[t] v[t+k], v[t] q[t+k] and
// q[t] q[t+k]: int64 [S][L + 1][4], every word written. The correlogram and the period are
// host arithmetic on these integers.
//
// A workgroup owns a share of consecutive chunks of kAutocorrChunk rows, a group of 8 series
// and a block of 256 lags. Per chunk it streams the chunk and the halo its lags reach from the
// time-major ring, quantises on load, and keeps one 16-bit word per sample (q, bit 15 =
// invalid) in LDS as [series][chunk + halo]; a thread owns 8 consecutive lags of one series and
// walks the chunk 8 rows at a time with the 8 + 16 words it needs in registers: 64 multiply-adds
// per two 16-byte LDS reads, int32 partials folded into 64 bits every 128 rows. A series without
// an invalid sample in the chunk and its halo takes n, Sx and Sy from prefix sums of q and runs
// the loop for Sxy alone; the others run it for all four. The destination is zeroed in stream
// order and the workgroups add their non-zero sums with vector 64-bit global integer atomics:
// exact, and the same bits in any order. No workspace, nothing allocated. 40.4 KB of LDS (the
// words of 8 series x 2064 rows, their block prefixes), 184 VGPRs, no scratch.
//
// Three entries over the one device routine:
//   * launch_autocorr_ring: one ring of series described by value;
//   * DeviceWindowSet::export_autocorr (device_window.h): the device rings of the last refresh;
//   * LongWindowSet::export_autocorr (long_window.h): the long windows of the last refresh.
#pragma once

#include <cstdint>

namespace rocmdash {

constexpr uint32_t kMaxAutocorrLags = 1024;       // L
constexpr uint32_t kMinAutocorrSpan = 1u << 6;    // span, a power of two
constexpr uint32_t kMaxAutocorrSpan = 1u << 20;
constexpr uint32_t kMaxAutocorrStride = 64;       // floats per ring row
constexpr uint32_t kAutocorrChunk = 1024;         // rows of a chunk (T)
constexpr uint32_t kAutocorrQMax = 4095;

inline bool bad_autocorr(uint32_t span, const float* scale, uint32_t L, const int64_t* dst) {
  return span < kMinAutocorrSpan || span > kMaxAutocorrSpan || (span & (span - 1)) != 0 || L < 1 || L > kMaxAutocorrLags ||
         scale == nullptr || dst == nullptr || (reinterpret_cast<uintptr_t>(dst) & 7u) != 0;
}

// base / stride / cols / depth / head / n as launch_bucket_ring (long_window_buckets.h); the
// span is the newest min(n, span) rows. scale: device [cols] floats, finite and > 0. dst: device
// [cols][L + 1][4] int64, 8-byte aligned, needs no initialisation. n == 0 or head == 0: all
// zeroes. Returns a hipError_t: hipErrorInvalidValue, before any launch or write, unless span is
// a power of two in [2^6, 2^20], 1 <= L <= 1024, launch_bucket_ring's ring conditions hold and
// base / scale / dst are set. share 0: the launch rule; else the chunks per workgroup, 1 <= share <= max(1, chunks).
int launch_autocorr_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                         uint32_t span, const float* scale, uint32_t L, int64_t* dst, void* stream, uint32_t share = 0);

}  // namespace rocmdash
