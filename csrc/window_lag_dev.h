// The lag walk of window_autocorr.hip, window_xcorr.hip and window_periods.hip. A workgroup of
// kThreads keeps kRows series of a chunk in LDS as 16-bit words [chunk + halo] (q in bits 0-11,
// bit 15 = no sample); a thread owns 8 consecutive lags of one row (against itself, or against a
// second row) and walks the chunk 8 rows at a time. Here, once: the LDS geometry, the word-level
// routines, the walk set with its unpack and its 8 x 8 mac, and the one-series tile and prefix.
// Each kernel keeps its own chunk loader, block prefix scan and per-thread step, and
// window_xcorr.hip its two-row tile over Sums: written as functions of this header (one tile over
// an accumulator type, a load and a scan stage), the same statements compile to other
// instruction streams for all three kernels under ROCm 7.2.0 - the one-series step as a function
// takes 188 VGPRs for 184 - and the one-series kernels then ran 0.4 - 0.8 % outside their parent's
// run-to-run spread on rows with NaN (profiles/lag_shared/). As it stands every kernel compiles
// to the instruction stream it had with its private copy.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "window_autocorr.h"
#include "window_xcorr_plan.h"  // for the static_assert on the geometry below, nothing else

namespace rocmdash {
namespace lag {

constexpr uint32_t kThreads = 256;     // 4 waves; under 256 VGPRs two waves share a SIMD, two workgroups a CU
constexpr uint32_t kRows = 8;          // LDS rows of a workgroup: one loader lane of every 8 each
constexpr uint32_t kT = kAutocorrChunk;  // rows of a chunk
constexpr uint32_t kKT = 8;            // consecutive lags a thread owns: one 16-byte LDS read
constexpr uint32_t kFold = 128;        // rows an int32 partial takes: 128 x 4095^2 < 2^31
constexpr uint32_t kInvalid = 0x8000u;  // bit 15 of a word: no sample (NaN, or past the rows' end)
constexpr uint32_t kPitch = kT + kMaxAutocorrLags + 16;  // words of an LDS row: chunk, halo, the last read's reach
constexpr uint32_t kBlocks = kPitch / 8;                 // 8-word blocks of a row
constexpr uint32_t kPBPitch = kBlocks + 2;
constexpr uint32_t kPerLane = (kBlocks + 63) / 64;  // blocks a lane sums in the prefix scan
static_assert(kPitch % 8 == 0 && (kPitch * 2) % 16 == 0 && kT % 16 == 0, "16-byte LDS reads");
static_assert(kPitch == kXcorrPitch && kThreads == kXcorrThreads && kKT == kXcorrLagTile,
              "the geometry window_xcorr_plan.h plans with on the host");
static_assert(uint64_t(kFold) * kAutocorrQMax * kAutocorrQMax < (1ull << 31), "an int32 partial, of q^2 x v too");

__device__ inline uint32_t lo12(uint32_t w) { return w & 0xfffu; }
__device__ inline uint32_t hi12(uint32_t w) { return (w >> 16) & 0xfffu; }

// a x b + c, a and b below 2^24: one full-rate instruction, and stated as one. Written as
// a * b + c or with __umul24, ROCm 7.2.0 (AMD clang 22.0.0git, roc-7.2.0) combines the chains of
// products of 12-bit fields into v_dot4_u32_u8, which keeps 8 bits of each factor: the sums of
// lags 1 - 3 and 5 - 7 of every 8 are short for q above 255. Plain C++ can return once a
// compiler no longer does that; tests/test_gpu_window_autocorr.py, test_gpu_window_xcorr.py and
// test_gpu_window_periods.py would each show it.
__device__ inline uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// the q of 8 consecutive words
__device__ inline void unpack_q(const uint4 p, uint32_t (&q)[8]) {
  const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    q[2 * i] = lo12(w[i]);
    q[2 * i + 1] = hi12(w[i]);
  }
}

// their validity: 1 for a sample, 0 for none
__device__ inline void unpack_v(const uint4 p, uint32_t (&v)[8]) {
  const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = (~w[i] >> 15) & 1u;
    v[2 * i + 1] = ~w[i] >> 31;
  }
}

// their q^2: below 2^24, so still a factor of mad24
__device__ inline void unpack_qq(const uint4 p, uint32_t (&s)[8]) {
  unpack_q(p, s);
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = mad24(s[i], s[i], 0u);
}

// What a walk over the chunk sums, as (p1, p2). kXY: (Sxy, -) - all a clean item needs from the
// loop. A marked series walks twice, kXYandY: (Sxy, Sy) and kNandX: (n | Sx << 8, -); a marked
// pair three times, kXYandY, kNXandXX: (n | Sx << 8, Sxx) and kYY: (Syy, -) - several walks so
// that each stays within the registers of kXYandY.
enum Walk { kXY, kXYandY, kNandX, kNXandXX, kYY };

// the x side of 8 rows: x1 multiplies into p1, x2 (kXYandY, kNXandXX) into p2
template <Walk kW>
__device__ inline void unpack_x(const uint4 p, uint32_t (&x1)[8], uint32_t (&x2)[8]) {
  if (kW == kYY) unpack_v(p, x1);
  if (kW != kYY) unpack_q(p, x1);
  if (kW == kXYandY) unpack_v(p, x2);
  if (kW == kNandX) {  // n in bits 0-7 (at most 128 per fold), Sx in bits 8-31 (at most 128 x 4095)
    unpack_v(p, x2);
#pragma unroll
    for (int i = 0; i < 8; ++i) x1[i] = x2[i] | (x1[i] << 8);
  }
  if (kW == kNXandXX) {  // p1 as kNandX, p2 from q^2
    uint32_t v[8];
    unpack_v(p, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      x2[i] = mad24(x1[i], x1[i], 0u);
      x1[i] = v[i] | (x1[i] << 8);
    }
  }
}

template <Walk kW>
__device__ inline void unpack_y(const uint4 p, uint32_t (&y)[8]) {
  if (kW == kNandX || kW == kNXandXX)
    unpack_v(p, y);
  else if (kW == kYY)
    unpack_qq(p, y);
  else
    unpack_q(p, y);
}

// 8 rows x 8 lags: x = rows t .. t + 7, (ya, yb) = rows t + k0 .. t + k0 + 15; every factor is below 2^24
template <Walk kW>
__device__ inline void mac(const uint32_t (&x1)[8], const uint32_t (&x2)[8], const uint32_t (&ya)[8], const uint32_t (&yb)[8],
                           uint32_t (&p1)[kKT], uint32_t (&p2)[kKT]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = 0; j < int(kKT); ++j) {
      const int e = i + j;
      const uint32_t y = e < 8 ? ya[e & 7] : yb[e & 7];
      p1[j] = mad24(x1[i], y, p1[j]);
      if (kW == kXYandY || kW == kNXandXX) p2[j] = mad24(x2[i], y, p2[j]);
    }
  }
}

// One thread's chunk: lags k0 .. k0 + 7 of the series at ws over rows [0, tend), tend a multiple
// of 16. Words past the rows' end are invalid with q = 0, so no row needs a bound. kXY and
// kXYandY add to (s1, s2) = (Sxy, Sy), kNandX to (n, Sx).
template <Walk kW>
__device__ inline void tile(const uint16_t* ws, uint32_t k0, uint32_t tend, uint64_t (&s1)[kKT], uint64_t (&s2)[kKT]) {
  const uint4* const xr = reinterpret_cast<const uint4*>(ws);
  const uint4* const yr = reinterpret_cast<const uint4*>(ws + k0);
  uint32_t ya[8], yb[8], x1[8], x2[8];
  unpack_y<kW>(yr[0], ya);
#pragma unroll 1
  for (uint32_t t = 0; t < tend; t += kFold) {
    uint32_t p1[kKT] = {}, p2[kKT] = {};
    const uint32_t ue = min(t + kFold, tend) >> 3;
#pragma unroll 1
    for (uint32_t u = t >> 3; u < ue; u += 2) {  // the window of 16 y slides by 8: (a, b) then (b, a)
      unpack_x<kW>(xr[u], x1, x2);
      unpack_y<kW>(yr[u + 1], yb);
      mac<kW>(x1, x2, ya, yb, p1, p2);
      unpack_x<kW>(xr[u + 1], x1, x2);
      unpack_y<kW>(yr[u + 2], ya);
      mac<kW>(x1, x2, yb, ya, p1, p2);
    }
#pragma unroll
    for (int j = 0; j < int(kKT); ++j) {
      if (kW == kNandX) {
        s1[j] += p1[j] & 0xffu;
        s2[j] += p1[j] >> 8;
      } else {
        s1[j] += p1[j];
        if (kW == kXYandY) s2[j] += p2[j];
      }
    }
  }
}

// sum of q over words [0, e) of a row: its block prefix and the first e % 8 words of the block
__device__ inline uint32_t prefix(const uint16_t* ws, const uint32_t* pbs, uint32_t e) {
  uint32_t q[8];
  unpack_q(reinterpret_cast<const uint4*>(ws)[e >> 3], q);
  uint32_t r = pbs[e >> 3];
#pragma unroll
  for (uint32_t i = 0; i < 7; ++i) r += i < (e & 7u) ? q[i] : 0u;
  return r;
}

}  // namespace lag
}  // namespace rocmdash
