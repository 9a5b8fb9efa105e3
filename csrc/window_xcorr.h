// Window cross-correlation: exact integer lead/lag sums of pairs of series of one ring - which
// of two series moves first, and by how many samples, which no export of one series and no
// joint histogram of one instant can tell. The semantics are stated once, in
// rocmdash/ops/window_xcorr.py: span, quantisation and scale are the autocorrelation's
// (window_autocorr.h); for 1 to 8 ordered pairs (a, b), a != b, both of one ring, and every lag
// k = -L .. L the output holds, over all t with 0 <= t < N and 0 <= t + k < N, the six sums of
// va[t] vb[t+k], qa[t] vb[t+k], va[t] qb[t+k], qa[t] qb[t+k], qa[t]^2 vb[t+k] and
// va[t] qb[t+k]^2: int64 [K][2L + 1][6], lag k at index L + k, every word written. The
// coefficient per lag and the lag of a pair are host arithmetic on these integers.
//
// A pair is two directed items, each summing x[t] against y[t + k] for k >= 0 only: (x = a,
// y = b) fills indices L .. 2L; (x = b, y = a), lags 1 .. L, fills indices L - 1 .. 0 with the x
// and the y words swapped on the store. A workgroup owns a share of consecutive chunks of
// kAutocorrChunk rows, up to 4 pairs and a block of 256 lags. Per chunk it reads the two columns
// of each pair over the chunk and the halo its lags reach from the time-major ring, quantises on
// load, and keeps one 16-bit word per sample (q, bit 15 = invalid) in LDS as 8 rows [chunk +
// halo]: row 2i is pair i's a, row 2i + 1 its b, and directed item r reads x from row r and y
// from row r ^ 1, so the 8 rows serve 8 items. A thread owns 8 consecutive lags of one item and
// walks the chunk 8 rows at a time with the 8 + 16 words it needs in registers, int32 partials
// folded every 128 rows (128 x 4095^2 < 2^31 also bounds the partials whose factor is q^2). An
// item whose two rows hold no invalid sample in the chunk and its halo takes n, Sx, Sy, Sxx and
// Syy from prefix sums - those of q in 32 bits, those of q^2 in 64: 2064 x 4095^2 is 3.5 x 10^10
// - and runs the loop for Sxy alone; the others walk three times for all six. n, Sx and Sy of a
// whole span fit 32 bits (4095 x 2^20 < 2^32) and are kept so; Sxy, Sxx and Syy in 64. The
// destination is zeroed in stream order and the workgroups add their non-zero sums with vector
// 64-bit global integer atomics: exact, and the same bits in any order. No workspace, nothing
// allocated. 58,016 B of LDS (the words of 8 rows x 2064 samples, their block prefixes of q and
// of q^2), 220 VGPRs (2 waves per SIMD, as the autocorrelation's 184), no scratch.
//
// Three entries over the one device routine:
//   * launch_xcorr_ring: one ring of series described by value;
//   * DeviceWindowSet::export_xcorr (device_window.h): the device rings of the last refresh;
//   * LongWindowSet::export_xcorr (long_window.h): the long windows of the last refresh.
#pragma once

#include <cstdint>

#include "window_autocorr.h"
#include "window_xcorr_plan.h"

namespace rocmdash {

static_assert(kXcorrChunk == kAutocorrChunk && kMaxXcorrLags == kMaxAutocorrLags && kMaxXcorrStride == kMaxAutocorrStride,
              "the cross-correlation's chunk, lags and stride are the autocorrelation's");

inline bool bad_xcorr(uint32_t span, const float* scale, const uint32_t* pairs, uint32_t K, uint32_t L, const int64_t* dst) {
  return bad_autocorr(span, scale, L, dst) || pairs == nullptr || K < 1 || K > kMaxXcorrPairs;
}

// base / stride / cols / depth / head / n / span / scale as launch_autocorr_ring. pairs: HOST
// [K][2] columns of the ring, 1 <= K <= 8, both below cols and a != b. dst: device
// [K][2L + 1][6] int64, 8-byte aligned, needs no initialisation. n == 0 or head == 0: all zeroes.
// Returns a hipError_t: hipErrorInvalidValue, before any launch or write, unless
// launch_autocorr_ring's conditions and these hold. share as launch_autocorr_ring: 0 is xcorr_share's rule.
int launch_xcorr_ring(const float* base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
                      uint32_t span, const float* scale, const uint32_t* pairs, uint32_t K, uint32_t L, int64_t* dst,
                      void* stream, uint32_t share = 0);

}  // namespace rocmdash
