// The long-window radix chain (long_window.h): pass 0..3 and scan 0..3, and the node
// chain's prediction and partials kernels.
//
// Adaptive digits. Only the key bits that vary over the window need resolving: bits
// above the highest differing bit of (min, max) and below the lowest bit any key
// differs in from a window member are shared by every sample. Pass 0 cannot know the
// exact range before it has read the window, so it predicts it from the previous
// refresh's exact min / max and the <= 256 rows that entered since (the window is a
// subset of the previous window and those rows, so the prediction is a superset of the
// varying bits: never wrong, at worst wider) and histograms the 10 (or 8, when 10 would
// not save a pass) bits just below the predicted top varying bit; without a prediction
// (first refresh, or more new rows than one workgroup reads) it takes the top key byte,
// as a fixed-digit radix select would. Passes 1..3 take 8-bit digits
// below it, down to the exact lowest varying bit; a series whose bits are all found
// skips the remaining passes, and a ring whose series all did exits at once. Integer
// telemetry in a band (temperatures, W, %) varies in <= 10 bits: one streaming pass
// instead of four; continuous data spans ~25 bits: three.

#include <stdexcept>

#include "long_window_pass.h"
#include "window_stats.h"

namespace rocmdash {
namespace {

// node mode, before pass 0: this rank's prediction of every series (one workgroup per
// ring segment) -> pred_local, all-gathered by the host between the launches
__global__ __launch_bounds__(NT) void lw_node_predict(const LwArgs a) {
  __shared__ uint32_t pmin[kSegCols], pmax[kSegCols], plo[kSegCols], plx[kSegCols], dref[kSegCols];
  if (blockIdx.x >= a.num_segs) return;  // uniform
  const LwSeg G = a.segs[blockIdx.x];
  const LwRing R = a.rings[G.ring];
  const uint32_t w = G.ncols, sb = R.first_series + G.col0;
  lw_predict(a, G.ring, R.dev + G.col0, R.width, w, sb, pmin, pmax, plo, plx, dref);
  const int t = threadIdx.x;
  if (uint32_t(t) < w) {
    LwPred p{};
    p.pmin = pmin[t];
    p.pmax = pmax[t];
    p.lo = min(plo[t], plx[t] ? uint32_t(__builtin_ctz(plx[t])) : 32u);
    p.ref = dref[t];
    p.has = a.params->n[G.ring] ? 1u : 0u;
    a.pred_local[sb + t] = p;
  }
}

// node mode, after pass 0: this rank's chunk partials of each series -> agg_local (one
// workgroup per series), all-gathered by the host; scan 0 then reduces the ranks' in rank
// order, so every rank holds the same node-wide count, sum, min, max and varying bits
__global__ __launch_bounds__(NT) void lw_node_partials(const LwArgs a) {
  __shared__ double dsum[NT];
  __shared__ uint32_t dcnt[NT], dmin[NT], dmax[NT], dor[NT], drf[NT];
  const uint32_t s = blockIdx.x;
  const LwPartial p =
      reduce_partials(a.part + size_t(s) * a.max_chunks, a.max_chunks, 1, dsum, dcnt, dmin, dmax, dor, drf);
  if (threadIdx.x == 0) a.agg_local[s] = p;
}

template <int PASS, int PF>
__global__ __launch_bounds__(NT) void lw_pass(const LwArgs a) {
  lw_pass_body<PASS, PF>(a);
}

// pass 3 over the candidates pass 2 kept (compaction on): one workgroup per (block of
// chunk_rows candidates, series); the same prefix test and LDS histogram as lw_pass<3>,
// merged into the same global histogram, so scan 3 does not know the difference
__global__ __launch_bounds__(NT) void lw_pass_cand(const LwArgs a) {
  __shared__ uint32_t h[kLongRanks * 128];
  __shared__ uint32_t pre_s[kLongRanks];
  const uint32_t s = blockIdx.y;
  const int t = threadIdx.x;
  const uint32_t wd = __builtin_amdgcn_readfirstlane(a.sel[s].width);
  if (!wd) return;  // resolved: nothing to count (uniform)
  // workgroup (c, s) reads the slab pass 2's workgroup c filled for series s
  const uint32_t rows = __builtin_amdgcn_readfirstlane(a.cand_n[size_t(s) * a.max_chunks + blockIdx.x]);
  if (!rows) return;
  uint32_t r, col;
  series_ring(a, s, r, col);
  const uint32_t row0 = blockIdx.x * a.rings[r].chunk_rows;
  const uint32_t fsh = __builtin_amdgcn_readfirstlane(a.sel[s].shift), dsh = fsh - wd;
  if (t < kLongRanks) pre_s[t] = a.sel[s].prefix[t] >> fsh;
  for (uint32_t i = t; i < kLongRanks * 128; i += NT) h[i] = 0;
  __syncthreads();
  uint32_t pre[kLongRanks], cmask = 0;
#pragma unroll
  for (int q = 0; q < kLongRanks; ++q) {
    pre[q] = pre_s[q];
    bool first = true;
#pragma unroll
    for (int q2 = 0; q2 < q; ++q2) first = first && pre[q2] != pre[q];
    if (first) cmask |= 1u << q;
  }
  const uint32_t* c = a.cand + size_t(s) * a.cand_cap + row0;
  for (uint32_t i = t; i < rows; i += NT) {
    const uint32_t k = c[i];
    const uint32_t bin = __builtin_amdgcn_ubfe(k, dsh, wd);
    const uint32_t hk = k >> fsh;
#pragma unroll
    for (int q = 0; q < kLongRanks; ++q)
      if (((cmask >> q) & 1u) && hk == pre[q]) atomicAdd(&h[q * 128 + (bin >> 1)], 1u << ((bin & 1u) * 16u));
  }
  __syncthreads();
  uint32_t* g = a.histk + size_t(s) * kLongRanks * 256;
  for (uint32_t i = t; i < kLongRanks * 128; i += NT) {
    const uint32_t x = h[i];
    if (x & 0xFFFFu) atomicAdd(&g[2 * i], x & 0xFFFFu);
    if (x >> 16) atomicAdd(&g[2 * i + 1], x >> 16);
  }
}

// ---- scan k: per series, find each rank's digit; the last scan writes the statistics ---
template <int PASS>
__global__ __launch_bounds__(NT) void lw_scan(const LwArgs a) {
  constexpr uint32_t BPT = PASS == 0 ? kB0 / NT : 1;  // bins per thread
  __shared__ uint32_t tmp[NT / 64];
  __shared__ double dsum[NT];
  __shared__ uint32_t dcnt[NT], dmin[NT], dmax[NT], dor[NT], drf[NT];
  __shared__ LwSel S;
  __shared__ uint32_t found_digit[kLongRanks], found_resid[kLongRanks];
  __shared__ uint32_t low_bits;  // the last scan: the key bits below the last digit (min's)
  const uint32_t s = blockIdx.x;
  const int t = threadIdx.x;
  if (a.brk_on && a.sel[s].done) return;  // scan B resolved the series (uniform)

  if constexpr (PASS == 0) {
    // partials in a fixed order -> deterministic mean (node mode: the ranks' all-gathered
    // partials in rank order - the same bits on every rank)
    const bool node = a.node_n != 0;
    const LwPartial tot = node ? reduce_partials(a.agg_all + s, a.node_n, a.num_series, dsum, dcnt, dmin, dmax, dor, drf)
                               : reduce_partials(a.part + size_t(s) * a.max_chunks, a.max_chunks, 1, dsum, dcnt, dmin,
                                                 dmax, dor, drf);
    if (t == 0) {
      S.nv = tot.cnt;
      S.done = 0;
      S.minkey = tot.minkey;
      S.maxkey = tot.maxkey;
      S.sum = tot.sum;
      S.shift = a.dig0[3 * s];
      S.width = a.dig0[3 * s + 2];  // this scan's digit: [shift, shift + width)
      // every key agrees with the reference key outside orx; bits above the predicted
      // range agree with min (the prediction is a superset of the varying bits)
      S.lo = tot.orx ? uint32_t(__builtin_ctz(tot.orx)) : 32u;
      uint32_t pos[kLongRanks];
      double frac[3];
      lw_positions(S.nv, a.params->pct, pos, frac);
      const uint32_t hb = S.shift + S.width;
      const uint32_t high = hb >= 32 ? 0u : (S.minkey >> hb) << hb;
      for (int q = 0; q < kLongRanks; ++q) {
        S.resid[q] = pos[q];
        S.prefix[q] = high;
      }
    }
  } else {
    if (t == 0) S = a.sel[s];
  }
  if (t < kLongRanks) {
    found_digit[t] = 0;
    found_resid[t] = 0;
  }
  __syncthreads();

  const uint32_t nv = S.nv;
  const bool search = nv && S.width;
  if (search) {
    for (int q = 0; q < kLongRanks; ++q) {
      // pass 0: every rank searches the one histogram of the series
      // passes > 0: ranks with one prefix share the histogram of the first of them
      int qc = q;
      if constexpr (PASS > 0) {
        for (int q2 = q - 1; q2 >= 0; --q2)
          if (S.prefix[q2] == S.prefix[q]) qc = q2;
      }
      const uint32_t* H = PASS == 0 ? a.hist0 + size_t(s) * kB0 : a.histk + (size_t(s) * kLongRanks + qc) * 256;
      uint32_t v[BPT], tot = 0;
#pragma unroll
      for (uint32_t j = 0; j < BPT; ++j) {
        v[j] = H[t * BPT + j];
        tot += v[j];
      }
      uint32_t excl, incl;
      block_scan(tot, tmp, excl, incl);
      const uint32_t rq = S.resid[q];
      if (tot && excl <= rq && rq < incl) {
#pragma unroll
        for (uint32_t j = 0; j < BPT; ++j) {
          if (v[j] && excl <= rq && rq < excl + v[j]) {
            found_digit[q] = t * BPT + j;
            found_resid[q] = rq - excl;
          }
          excl += v[j];
        }
      }
      __syncthreads();
    }
  }
  // re-zero what this scan consumed (the next pass / refresh accumulates into it)
  if constexpr (PASS == 0) {
#pragma unroll
    for (uint32_t j = 0; j < BPT; ++j) a.hist0[size_t(s) * kB0 + t * BPT + j] = 0;
  } else {
    for (int q = 0; q < kLongRanks; ++q) a.histk[(size_t(s) * kLongRanks + q) * 256 + t] = 0;
  }
  if (t == 0) {
    if (search) {
      for (int q = 0; q < kLongRanks; ++q) {
        S.prefix[q] |= found_digit[q] << (PASS == 0 ? S.shift : S.shift - S.width);
        S.resid[q] = found_resid[q];
      }
    }
    if constexpr (PASS > 0) S.shift -= S.width;
    S.width = nv ? next_width(S.shift, S.lo) : 0u;
    // bits below the last digit never vary: min's (shift <= 22 here)
    low_bits = S.minkey & ~(0xFFFFFFFFu << S.shift);
  }
  __syncthreads();
  if constexpr (PASS < 3) {
    if (t == 0) a.sel[s] = S;
  } else {
    if (t == 0) {
      a.sel[s] = S;  // min / max: the next refresh's prediction
      // the next refresh's brackets around the percentile keys just found
      uint32_t klo[kBrkQ], khi[kBrkQ];
      for (int q = 0; q < kBrkQ; ++q) {
        klo[q] = S.prefix[2 * q] | low_bits;
        khi[q] = S.prefix[2 * q + 1] | low_bits;
      }
      LwBrk b = a.brk[s];
      const bool had = a.brk_on && b.valid;
      const float est = lw_brk_est(S.minkey, S.maxkey, nv, lw_brk_target(a, nv));
      for (int q = 0; q < kBrkQ; ++q) {
        lw_next_bracket(b.delta[q], b.cin[q], b.lo[q], b.hi[q], klo[q], khi[q], est, had, lw_brk_target(a, nv),
                        !b.nounion[q], &b.dsave[q]);
        b.nounion[q] = 0u;
      }
      // incremental mode: brackets pay for every series (pass B then streams only the
      // chunks that changed); else only where the radix chain needs > 1 streaming pass
      b.valid = a.incr ? (nv ? 1u : 0u) : lw_brk_wanted(nv, S.minkey, S.maxkey, S.lo);
      b.hit = 0;
      a.brk[s] = b;
      if (a.hflags) a.hflags[s] = b.valid;  // the host's hint: launch pass B next refresh
      if (a.bchg) a.bchg[s] = 1u;  // new brackets: every chunk's counts must be taken again
    }
    if (t < STAT_NUM) {
      uint32_t r, col;
      series_ring(a, s, r, col);
      const LwRing R = a.rings[r];
      const uint64_t head = a.params->head[r];
      const uint32_t n = a.params->n[r];
      float o = __builtin_nanf("");
      if (t == STAT_COUNT) {
        o = float(nv);
      } else if (t == STAT_LAST) {  // node mode: no node-wide newest sample (NaN)
        if (n && !a.node_n) o = R.dev[((head - 1) & uint64_t(a.mask)) * R.width + col];
      } else if (nv) {
        if (t == STAT_MIN) {
          o = kfloat(S.minkey);
        } else if (t == STAT_MAX) {
          o = kfloat(S.maxkey);
        } else if (t == STAT_MEAN) {
          o = float(S.sum / double(nv));
        } else {
          const int q = t - STAT_P0;
          uint32_t pos[kLongRanks];
          double frac[3];
          lw_positions(nv, a.params->pct, pos, frac);
          const double x0 = kfloat(S.prefix[2 * q] | low_bits), x1 = kfloat(S.prefix[2 * q + 1] | low_bits);
          const double f = frac[q];
          o = float(f >= 0.5 ? x1 - (x1 - x0) * (1.0 - f) : x0 + (x1 - x0) * f);
        }
      }
      a.out[size_t(s) * STAT_NUM + t] = o;
    }
  }
}

template <int PASS>
void launch_pass(int prefetch, dim3 grid, size_t lds, hipStream_t stream, const LwArgs& a) {
  if (prefetch == 1) hipLaunchKernelGGL((lw_pass<PASS, 1>), grid, dim3(NT), lds, stream, a);
  else if (prefetch == 2) hipLaunchKernelGGL((lw_pass<PASS, 2>), grid, dim3(NT), lds, stream, a);
  else hipLaunchKernelGGL((lw_pass<PASS, 0>), grid, dim3(NT), lds, stream, a);
}

}  // namespace

void lw_launch_node_predict(hipStream_t stream, const LwArgs& a) {
  hipLaunchKernelGGL(lw_node_predict, dim3(a.num_segs), dim3(NT), 0, stream, a);
}

void lw_launch_node_partials(hipStream_t stream, const LwArgs& a) {
  hipLaunchKernelGGL(lw_node_partials, dim3(a.num_series), dim3(NT), 0, stream, a);
}

void lw_launch_pass(int pass, int prefetch, uint32_t grid, size_t lds, hipStream_t stream, const LwArgs& a) {
  switch (pass) {
    case 0: return launch_pass<0>(prefetch, dim3(grid), lds, stream, a);
    case 1: return launch_pass<1>(prefetch, dim3(grid), lds, stream, a);
    case 2: return launch_pass<2>(prefetch, dim3(grid), lds, stream, a);
    case 3: return launch_pass<3>(prefetch, dim3(grid), lds, stream, a);
    default: throw std::logic_error("long window: pass 0..3");
  }
}

void lw_launch_pass_cand(hipStream_t stream, const LwArgs& a) {
  hipLaunchKernelGGL(lw_pass_cand, dim3(a.max_chunks, a.num_series), dim3(NT), 0, stream, a);
}

void lw_launch_scan(int pass, hipStream_t stream, const LwArgs& a) {
  const dim3 grid(a.num_series);
  switch (pass) {
    case 0: hipLaunchKernelGGL(lw_scan<0>, grid, dim3(NT), 0, stream, a); return;
    case 1: hipLaunchKernelGGL(lw_scan<1>, grid, dim3(NT), 0, stream, a); return;
    case 2: hipLaunchKernelGGL(lw_scan<2>, grid, dim3(NT), 0, stream, a); return;
    case 3: hipLaunchKernelGGL(lw_scan<3>, grid, dim3(NT), 0, stream, a); return;
    default: throw std::logic_error("long window: scan 0..3");
  }
}

}  // namespace rocmdash
