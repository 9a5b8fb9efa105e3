// Device helpers more than one long-window kernel file uses: the order-preserving key,
// percentile positions, the fixed-order reductions and block scans, and the bracket-sizing
// rules that both the radix chain's last scan and scan B apply.
#pragma once

#include "long_window_args.h"

namespace rocmdash {
// Internal linkage (an anonymous namespace, as in a single file): each kernel file is its own
// device program, and a function-local __shared__ array of a function with external linkage
// stays in every kernel that inlines it, read or not (32 B of LDS in the passes that keep
// no candidate counts).
namespace {

// a += b (partials of disjoint sample sets), sums added in the caller's fixed order
__device__ __forceinline__ void lw_combine(double& sm, uint32_t& cn, uint32_t& lo, uint32_t& hi, uint32_t& ox,
                                           uint32_t& rf, double bs, uint32_t bc, uint32_t bl, uint32_t bh, uint32_t bo,
                                           uint32_t br) {
  sm += bs;
  if (bc) {
    if (cn) {
      ox |= bo | (br ^ rf);
    } else {
      ox = bo;
      rf = br;
    }
    cn += bc;
    lo = min(lo, bl);
    hi = max(hi, bh);
  }
}

__device__ inline uint32_t eq_lo(uint32_t e) { return e & 0xFFFFu; }
__device__ inline uint32_t eq_hi(uint32_t e) { return e >> 16; }

// order-preserving float <-> uint32 key (NaN never keyed: callers skip it)
__device__ __forceinline__ uint32_t fkey(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float kfloat(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// sorted positions [lo0, hi0, lo1, hi1, lo2, hi2] and interpolation weights of the
// three percentiles over nv valid samples (numpy 'linear', as window_stats.hip)
__device__ inline void lw_positions(uint32_t nv, const float pct[3], uint32_t (&pos)[kLongRanks], double (&frac)[3]) {
  const uint32_t last = nv ? nv - 1 : 0;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double p = double(pct[q]) / 100.0 * double(last);
    uint32_t lo = uint32_t(floor(p));
    if (lo > last) lo = last;
    pos[2 * q] = lo;
    pos[2 * q + 1] = lo + 1 < nv ? lo + 1 : last;
    frac[q] = double(float(p - double(lo)));  // float weight, as the LDS kernel
  }
}

__device__ inline void series_ring(const LwArgs& a, uint32_t s, uint32_t& r, uint32_t& col) {
  r = 0;
  for (uint32_t i = 0; i < a.num_rings; ++i)
    if (s >= a.rings[i].first_series) r = i;
  col = s - a.rings[r].first_series;
}

// width of the digit below `shift` when bits below `lo` never vary: <= 8 bits, 0 = done
__device__ __forceinline__ uint32_t next_width(uint32_t shift, uint32_t lo) {
  return shift > lo ? min(8u, shift - lo) : 0u;
}

// The block's reduction of per-thread combined partials (thread order fixed: butterflies,
// then the waves in order) - every caller's partials reduce to the same bits.
__device__ inline LwPartial block_reduce_partial(double sm, uint32_t cn, uint32_t lo, uint32_t hi, uint32_t ox,
                                                 uint32_t rf, double* dsum, uint32_t* dcnt, uint32_t* dmin,
                                                 uint32_t* dmax, uint32_t* dor, uint32_t* dref) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  (void)t;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double os = __shfl_xor(sm, off);
    const uint32_t oc = uint32_t(__shfl_xor(int(cn), off)), ol = uint32_t(__shfl_xor(int(lo), off)),
                   oh = uint32_t(__shfl_xor(int(hi), off)), oo = uint32_t(__shfl_xor(int(ox), off)),
                   orf = uint32_t(__shfl_xor(int(rf), off));
    lw_combine(sm, cn, lo, hi, ox, rf, os, oc, ol, oh, oo, orf);
  }
  if (lane == 0) {
    dsum[wave] = sm;
    dcnt[wave] = cn;
    dmin[wave] = lo;
    dmax[wave] = hi;
    dor[wave] = ox;
    dref[wave] = rf;
  }
  __syncthreads();
  LwPartial r{0.0, 0, 0xFFFFFFFFu, 0, 0, 0, 0};
  for (int wv = 0; wv < NT / 64; ++wv)
    lw_combine(r.sum, r.cnt, r.minkey, r.maxkey, r.orx, r.ref, dsum[wv], dcnt[wv], dmin[wv], dmax[wv], dor[wv],
               dref[wv]);
  __syncthreads();  // the arrays are reusable
  return r;
}

// one series' partials over `count` entries (stride apart) in a fixed order: per thread
// in index order, a wave butterfly (both partners add the same pair: every lane holds the
// same bits), then the 4 waves in order -> every thread (deterministic sum)
__device__ inline LwPartial reduce_partials(const LwPartial* P, uint32_t count, uint32_t stride, double* dsum,
                                            uint32_t* dcnt, uint32_t* dmin, uint32_t* dmax, uint32_t* dor,
                                            uint32_t* dref) {
  const int t = threadIdx.x;
  double sm = 0.0;
  uint32_t cn = 0, lo = 0xFFFFFFFFu, hi = 0, ox = 0, rf = 0;
  for (uint32_t i = t; i < count; i += NT) {
    const LwPartial pp = P[size_t(i) * stride];
    lw_combine(sm, cn, lo, hi, ox, rf, pp.sum, pp.cnt, pp.minkey, pp.maxkey, pp.orx, pp.ref);
  }
  return block_reduce_partial(sm, cn, lo, hi, ox, rf, dsum, dcnt, dmin, dmax, dor, dref);
}

// exclusive / inclusive prefix of one value per thread over the 256-thread block
__device__ inline void block_scan(uint32_t v, uint32_t* tmp, uint32_t& excl, uint32_t& incl) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(x, off);
    if (lane >= off) x += y;
  }
  if (lane == 63) tmp[wave] = x;
  __syncthreads();
  uint32_t base = 0;
  for (int wv = 0; wv < wave; ++wv) base += tmp[wv];
  incl = base + x;
  excl = incl - v;
  __syncthreads();  // tmp reusable
}

// exclusive / inclusive prefix of one value per thread over the 256-thread block; total:
// the block's sum (every thread)
__device__ inline void block_scan_total(uint32_t v, uint32_t* tmp, uint32_t& excl, uint32_t& incl, uint32_t& total) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(x, off);
    if (lane >= off) x += y;
  }
  if (lane == 63) tmp[wave] = x;
  __syncthreads();
  uint32_t base = 0, tot = 0;
  for (int wv = 0; wv < NT / 64; ++wv) {
    if (wv < wave) base += tmp[wv];
    tot += tmp[wv];
  }
  incl = base + x;
  excl = incl - v;
  total = tot;
  __syncthreads();  // tmp reusable
}

// The next refresh's bracket q: around this refresh's percentile keys (its lo / hi
// position), half-width adapted so the bracket holds ~kBrkTarget samples. `had`: the
// bracket was used this refresh and b.cin[q] holds what it held (else a first estimate
// `est` from the key range: uniform density over [min, max]).
// samples a bracket aims to hold: kBrkTarget, or 1/16 of a small window (a chunk's slab
// keeps at most a quarter of its rows per bracket)
__device__ inline uint32_t lw_brk_target(const LwArgs& a, uint32_t nv) {
  return max(64u, min(a.node_brk ? kNodeBrkTarget : a.brk_target, nv / 16));
}
// The half-width is kept in value units: the number of samples inside grows linearly with
// it there, while in key units it does not (near 0 a key step is a tiny value step, far
// from it a large one: mixed-sign data centred on 0 made a key-unit half-width oscillate
// between a few hundred and tens of thousands of samples)
// The first estimate assumes a quarter of the uniform density's width: near a normal
// distribution's median the density is ~3x the uniform one over [min, max], and a first
// bracket that overflows its kept-key cap is read as ties (below)
__device__ inline float lw_brk_est(uint32_t minkey, uint32_t maxkey, uint32_t nv, uint32_t target) {
  if (!nv) return 0.f;
  const double est = (double(kfloat(maxkey)) - double(kfloat(minkey))) * double(target) / (8.0 * nv);
  return est > 0.0 && est < 3.0e38 ? float(est) : (est > 0.0 ? 3.0e38f : 0.f);
}
// delta (float bits) / cin: the bracket's half-width and what it held this refresh -> its
// next half-width and bounds (delta, lo, hi updated in place); a half-width of 0 makes the
// bracket exactly [klo, khi] (ties: a one-key bracket stores no keys)
__device__ inline void lw_next_bracket(uint32_t& delta, uint32_t cin, uint32_t& lo, uint32_t& hi, uint32_t klo,
                                       uint32_t khi, float est, bool had, uint32_t target, bool join = true,
                                       uint32_t* dsave = nullptr) {
  const float dv = __uint_as_float(delta);
  double d;
  if (!had) {
    d = est;
  } else if (dv == 0.f) {  // an exact-key bracket: keep it while ties hold the rank
    if (cin >= target / 8) {
      // the percentile moved to a neighbouring tied value (a median between two readings
      // flips between them): the next exact bracket spans the old keys and the new, and
      // holds both with their ties counted on its bounds. Not after an overflow (a value
      // between them had too many ties to keep): then only the new keys
      if (join) {
        lo = min(lo, klo);
        hi = max(hi, khi);
      } else {
        lo = klo;
        hi = khi;
      }
      return;
    }
    // not ties after all (an overflow read as ties on continuous data with heavy tails):
    // back to the value half-width the overflow put aside, else the estimate
    const float ds = dsave ? __uint_as_float(*dsave) : 0.f;
    d = ds > 0.f ? double(ds) : double(est);
  } else {
    // to the target in one step when it held too many (the local density), at most 8x
    // wider when too few
    d = double(dv) * fmin(8.0, double(target) / double(max(cin, 1u)));
  }
  if (dsave) *dsave = 0u;
  if (!(d < 3.0e38)) d = 3.0e38;
  const float df = float(d);
  delta = __float_as_uint(df);
  if (df == 0.f) {
    lo = klo;
    hi = khi;
    return;
  }
  lo = min(klo, fkey(kfloat(klo) - df));  // rounding never leaves the keys outside
  hi = max(khi, fkey(kfloat(khi) + df));
  if (klo - lo <= 1u && hi - khi <= 1u) {
    // narrower than the keys' spacing: ties (a bracket around tied values keeps every tie
    // and overflows, shrinking it further cannot help) - exactly the keys, whose ties are
    // then counted on the bounds instead of kept
    delta = 0u;
    lo = klo;
    hi = khi;
  }
}
// Brackets pay when the radix chain needs more than one streaming pass: a window whose
// varying key bits [lo, top] span <= 10 bits (integer telemetry in a band) is resolved
// by pass 0's digit alone, which costs less than pass B
__device__ inline uint32_t lw_brk_wanted(uint32_t nv, uint32_t minkey, uint32_t maxkey, uint32_t lo) {
  const uint32_t d = minkey ^ maxkey;
  const uint32_t top = d ? 31u - uint32_t(__builtin_clz(d)) : 0u;
  const uint32_t span = top >= lo ? top - lo + 1 : 1u;
  return nv && span > uint32_t(kD0) ? 1u : 0u;
}

}  // namespace
}  // namespace rocmdash
