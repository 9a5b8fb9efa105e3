// The streaming body shared by the radix passes, pass B and the fused scan B: one
// workgroup streams one chunk of one ring segment (pass_chunk), lw_pass_body sets it up
// and merges what it counted.
#pragma once

#include "long_window_dev.h"

namespace rocmdash {
namespace {  // internal linkage: see long_window_dev.h

// LDS histograms hold two 16-bit bins per word (a chunk has <= kLongChunkRowsMax < 2^16
// rows, so a bin never overflows into its neighbour), sized at launch for the widest ring:
// pass 0 [width][kB0 / 2] words (32 KB for 16 series), passes k [width][6 ranks][128] words.
//
// The stream is latency-bound, not bandwidth-bound, at the few waves per CU a window's
// chunks give: each thread therefore issues the loads of U rows (U x WM floats in
// registers, WM = the ring width rounded up to 4 / 8 / 16, chosen per ring by a uniform
// branch) before it histograms any of them. Ranks whose prefixes agree (the lo / hi
// positions of one percentile usually do) share one histogram: only the first rank
// of each prefix counts (cmask), the scan reads that rank's histogram for the others.
//
// Pass 0 adds a wave's count with one atomic for the lanes that share the first lane's
// bin, one atomic per sample for the others. Measured and rejected: the general form
// (a ballot per distinct bin, up to 3 rounds, in every pass) cost more VALU than the
// conflicts it removed - 2.6x slower overall at W = 2^20
// (profiles/r01/long_window_profile.json).
struct LwShared {
  const uint32_t* pre;    // [width][kLongRanks] prefixes of the ranks (passes > 0)
  const uint32_t* shift;  // [width] pass 0: digit shift; passes > 0: found-bits shift
  const uint32_t* width;  // [width] passes > 0: digit width (0 = resolved)
  const uint32_t* ref;    // [width] pass 0: the reference key of orx
  double (*rsum)[kSegCols];
  uint32_t (*rcnt)[kSegCols];
  uint32_t (*rmin)[kSegCols];
  uint32_t (*rmax)[kSegCols];
  uint32_t (*ror)[kSegCols];
  uint32_t* ccount;  // pass 2 compaction: candidates of each series in this chunk (LDS)
  uint32_t colmask;  // pass 0 / B: the segment's series this pass works on (bit per column)
  uint32_t* bcnt;    // pass B: samples strictly inside each (column, bracket) in this chunk (LDS)
  uint32_t* beq;     // pass B: samples on each (column, bracket)'s bounds, packed as LwBrkPart::eq (LDS)
  uint32_t (*rlt)[kSegCols * kBrkQ];  // pass B: per-wave below-bracket counts
};

struct LwView {  // one segment of one ring
  const float* dev;  // the ring's window + the segment's first column
  uint32_t stride;   // floats per row (the ring's width)
  uint32_t chunk_rows;  // the ring's rows per workgroup
  uint32_t nc;       // series in the segment (<= kSegCols)
  bool vec;          // 16-byte aligned float4 loads
  uint32_t sb;       // the segment's first series
  uint32_t* bkeys;   // pass B: the segment's first series' kept-key slabs
  uint64_t bstride;  // keys per series
  uint32_t qcap;     // keys per (chunk, bracket)
  const LwBrk* brk;  // pass B: the brackets it counts against (brk; the fused pass: brk_used)
  uint32_t qkeys;    // pass B: brackets whose kept keys it stores (bit per bracket)
  // the fused pass B (one column): orx's reference read here, after the rows' loads are in
  // flight (one memory latency for both), instead of from LDS (sh_.ref); its key -> *ref_out
  const float* newest;  // the column's newest sample (nullptr: none / not fused)
  bool fused_ref;
  uint32_t* ref_out;    // LDS
};

// PF: the thread's next U rows are loaded before this iteration's samples are counted
// (two register buffers), so the loads are in flight while the wave computes. A compile-
// time choice: a runtime switch would make every pass kernel carry the registers of both.
template <int PASS, int WM, int U, bool PF, int UG = (WM <= 4 ? 8 : 4)>
__device__ __forceinline__ void pass_chunk(const LwArgs& a, const LwView& V, uint32_t r, uint32_t c, uint32_t* h,
                                           uint32_t hw, const LwShared& sh_) {
  const uint32_t w = V.nc;  // <= WM
  // Chunks are PHYSICAL: chunk c is the device ring's slots [c x chunk_rows, ..) - rows that
  // entered the window overwrite the slots of rows that left, so a refresh changes only
  // the chunks its new rows landed in and every other chunk's partials / bracket counts
  // stay valid (incremental pass B). The window is the set of its slots: slots a filling
  // window has not reached yet hold NaN (never counted), like failed reads.
  const uint32_t wslots = a.mask + 1u;
  const uint32_t row0 = c * V.chunk_rows;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const uint32_t rows = row0 < wslots ? min(wslots - row0, V.chunk_rows) : 0u;
  (void)r;

  double sum[WM];
  uint32_t cnt[WM], mn[WM], mx[WM], orx[WM];
  uint32_t dsh[WM], dwd[WM], fsh[WM], ref[WM];  // workgroup-uniform: scalar registers
  uint32_t pre[WM][kLongRanks];  // passes > 0: the rank's found bits (prefix >> fsh)
  uint32_t cmask[WM];  // ranks that own a histogram (first of each distinct prefix)
  // pass B: per lane, the samples below each bracket; narrow variants (<= 4 columns) also
  // count the samples on its bounds here (lo | hi << 16), wide ones with LDS atomics
  constexpr bool EQREG = WM <= 4;
  uint32_t lt[WM][kBrkQ];
  uint32_t eqr[EQREG ? WM : 1][kBrkQ];
  const uint32_t colmask = sh_.colmask;
  const uint32_t qcap = V.qcap;  // pass B: kept keys per (chunk, bracket) slab
#pragma unroll
  for (int col = 0; col < WM; ++col) {
    sum[col] = 0.0;
    cnt[col] = 0;
    mn[col] = 0xFFFFFFFFu;
    mx[col] = 0;
    orx[col] = 0;
    cmask[col] = 0;
    dsh[col] = fsh[col] = ref[col] = dwd[col] = 0;
#pragma unroll
    for (int q = 0; q < kBrkQ; ++q) {
      lt[col][q] = 0;
      if constexpr (EQREG) eqr[col][q] = 0;
    }
    if (uint32_t(col) < w) {
      if constexpr (PASS == kPassBrk) {
        if (!V.fused_ref) ref[col] = __builtin_amdgcn_readfirstlane(sh_.ref[col]);  // bounds: per column in the loop
      } else if constexpr (PASS == 0) {
        dsh[col] = __builtin_amdgcn_readfirstlane(sh_.shift[col]);
        ref[col] = __builtin_amdgcn_readfirstlane(sh_.ref[col]);
        dwd[col] = __builtin_amdgcn_readfirstlane(sh_.width[col]);
      } else {
        const uint32_t wd = __builtin_amdgcn_readfirstlane(sh_.width[col]);
        fsh[col] = __builtin_amdgcn_readfirstlane(sh_.shift[col]);
        dsh[col] = fsh[col] - wd;
        dwd[col] = wd;
        if (wd) {
#pragma unroll
          for (int q = 0; q < kLongRanks; ++q) {
            pre[col][q] = sh_.pre[col * kLongRanks + q] >> fsh[col];
            bool first = true;
#pragma unroll
            for (int q2 = 0; q2 < q; ++q2) first = first && pre[col][q2] != pre[col][q];
            if (first) cmask[col] |= 1u << q;
          }
        }
      }
    }
  }
  const bool vec = V.vec;
  // the U rows of a thread's next iteration are loaded before this iteration's samples
  // are counted (a.prefetch): the loads are in flight while the wave computes, instead of
  // the wave's memory pipe idling through every counting phase
  const auto load_rows = [&](float (&dst)[U][WM], uint32_t i0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = i0 + uint32_t(u) * NT;
      const float* p = V.dev + size_t(row0 + i) * V.stride;
      if (i < rows && vec) {
#pragma unroll
        for (int q4 = 0; q4 < WM / 4; ++q4) {
          if (uint32_t(4 * q4) < w) {
            const float4 f = reinterpret_cast<const float4*>(p)[q4];
            dst[u][4 * q4] = f.x;
            dst[u][4 * q4 + 1] = f.y;
            dst[u][4 * q4 + 2] = f.z;
            dst[u][4 * q4 + 3] = f.w;
          }
        }
      } else {
#pragma unroll
        for (int col = 0; col < WM; ++col) dst[u][col] = (i < rows && uint32_t(col) < w) ? p[col] : __builtin_nanf("");
      }
    }
  };
  constexpr bool pf = PF;
  float v[U][WM], vn[U][WM];
  // pass 0 / B: a thread's values of a series are summed in fp32 over groups of UG rows
  // (its rows i0 + u x NT in order), then added to the fp64 total once per group (a
  // quarter of the fp64 adds; <= UG terms per fp32 partial). UG is fixed by the segment
  // width, not by U, so every pass variant sums the same groups: the same mean bits
  // (a column-split pass B - WM 1 - takes its segment's UG: the same groups, the same sums).
  // U > UG (the column-split pass B: many rows in flight per thread) flushes every UG rows
  // inside the iteration - the same groups
  static_assert(UG % U == 0 || (U % UG == 0 && WM == 1 && PASS == kPassBrk), "rows per sum group");
  constexpr bool INNER_FLUSH = U > UG;
  float psum[WM];
#pragma unroll
  for (int col = 0; col < WM; ++col) psum[col] = 0.f;
  int git = 0;  // iterations into the current group
  const auto flush = [&]() {
#pragma unroll
    for (int col = 0; col < WM; ++col) {
      sum[col] += double(psum[col]);
      psum[col] = 0.f;
    }
  };
  if (uint32_t(t) < rows) load_rows(v, uint32_t(t));
  if constexpr (PASS == kPassBrk) {
    if (V.fused_ref) {  // one column (WM 1): its newest sample's key, loaded behind the rows
      const float xn = V.newest ? *V.newest : __builtin_nanf("");
      ref[0] = isnan(xn) ? 0u : fkey(xn);
      if (t == 0) *V.ref_out = ref[0];
    }
  }
  for (uint32_t i0 = uint32_t(t); i0 < rows; i0 += NT * U) {
    const uint32_t inext = i0 + NT * U;
    if constexpr (pf) {
      if (inext < rows) load_rows(vn, inext);
    }
    if constexpr (PASS == kPassBrk) {
      // pass B, column by column: the column's bounds once per iteration, then its U
      // samples
#pragma unroll
      for (int col = 0; col < WM; ++col) {
        if (uint32_t(col) < w && ((colmask >> col) & 1u)) {  // uniform
          // this refresh's brackets of the column: read through the constant address space
          // (scalar loads - nothing writes brk while pass B runs), here in the loop, not
          // hoisted: 8 columns' bounds held across the loop spill
          asm volatile("" ::: "memory");
          typedef const __attribute__((address_space(4))) uint32_t* cptr;
          const cptr cb = (cptr)(V.brk + V.sb + col);  // LwBrk: lo[3], hi[3], ...
          const uint32_t l0 = cb[0], l1 = cb[1], l2 = cb[2], h0 = cb[3], h1 = cb[4], h2 = cb[5];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if constexpr (INNER_FLUSH) {
              if (u && u % UG == 0) {  // a group of UG rows done (uniform: u is unrolled)
                sum[col] += double(psum[col]);
                psum[col] = 0.f;
              }
            }
            const float x = v[u][col];
            if (isnan(x)) continue;  // failed reads, rows past the chunk
            const uint32_t k = fkey(x);
            psum[col] += x;
            ++cnt[col];
            mn[col] = min(mn[col], k);
            mx[col] = max(mx[col], k);
            orx[col] |= k ^ ref[col];
            const bool b0 = k < l0, b1 = k < l1, b2 = k < l2;
            lt[col][0] += b0 ? 1u : 0u;
            lt[col][1] += b1 ? 1u : 0u;
            lt[col][2] += b2 ? 1u : 0u;
            // inside a bracket: rare for continuous data (a bracket holds ~kBrkTarget of
            // the window's samples). On a bound - counted, not kept: a bracket whose bounds
            // are tied values (a percentile of telemetry readings) then holds the rank with
            // no keys at all, however many samples tie. Strictly inside: per bracket, the
            // wave's count goes to the chunk's LDS counter and its keys to the slab
            const bool i0 = !b0 && k <= h0, i1 = !b1 && k <= h1, i2 = !b2 && k <= h2;
            const bool e0 = i0 && (k == l0 || k == h0), e1 = i1 && (k == l1 || k == h1),
                       e2 = i2 && (k == l2 || k == h2);
            if constexpr (EQREG) {  // per-lane counters: no ballots for ties
              eqr[col][0] += e0 ? (k == l0 ? 1u : 0x10000u) : 0u;
              eqr[col][1] += e1 ? (k == l1 ? 1u : 0x10000u) : 0u;
              eqr[col][2] += e2 ? (k == l2 ? 1u : 0x10000u) : 0u;
            } else if (__ballot(e0 || e1 || e2)) {
#pragma unroll
              for (int q = 0; q < kBrkQ; ++q) {
                const uint32_t lo = q == 0 ? l0 : (q == 1 ? l1 : l2);
                const bool onb = q == 0 ? e0 : (q == 1 ? e1 : e2);
                const uint64_t me = __ballot(onb);
                if (me) {
                  const uint32_t nlo = uint32_t(__popcll(__ballot(onb && k == lo)));
                  if (lane == __builtin_ctzll(me))
                    atomicAdd(&sh_.beq[col * kBrkQ + q], nlo | ((uint32_t(__popcll(me)) - nlo) << 16));  // LDS
                }
              }
            }
            const bool m0 = i0 && !e0, m1 = i1 && !e1, m2 = i2 && !e2;
            if (__ballot(m0 || m1 || m2)) {
#pragma unroll
              for (int q = 0; q < kBrkQ; ++q) {
                const bool mid = q == 0 ? m0 : (q == 1 ? m1 : m2);
                const uint64_t mb = __ballot(mid);
                if (mb) {
                  const int leader = __builtin_ctzll(mb);
                  uint32_t base = 0;
                  if (lane == leader) base = atomicAdd(&sh_.bcnt[col * kBrkQ + q], uint32_t(__popcll(mb)));  // LDS
                  base = uint32_t(__builtin_amdgcn_readlane(int(base), leader));
                  if (mid) {
                    const uint32_t slot =
                        base + __builtin_amdgcn_mbcnt_hi(uint32_t(mb >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mb), 0u));
                    if (slot < qcap && ((V.qkeys >> q) & 1u))  // a fuller slab: scan B sees mid > qcap, the chain
                      V.bkeys[size_t(col) * V.bstride + (size_t(c) * kBrkQ + q) * qcap + slot] = k;
                  }
                }
              }
            }
          }
        }
      }
    } else {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int col = 0; col < WM; ++col) {
        if (uint32_t(col) < w && ((colmask >> col) & 1u)) {  // uniform: w is the segment's
          const float x = v[u][col];
          if (isnan(x)) continue;  // failed reads, rows past the chunk
          const uint32_t k = fkey(x);
          const uint32_t bin = __builtin_amdgcn_ubfe(k, dsh[col], dwd[col]);  // one v_bfe_u32
          if constexpr (PASS == 0) {
            psum[col] += x;
            ++cnt[col];
            mn[col] = min(mn[col], k);
            mx[col] = max(mx[col], k);
            orx[col] |= k ^ ref[col];
            // the first lane's bin is added as one count for every lane that shares it,
            // only lanes with another bin add one each
            const uint64_t act = __ballot(1);  // the lanes here: valid samples
            const int first = __builtin_ctzll(act);
            const uint32_t lb = uint32_t(__builtin_amdgcn_readlane(int(bin), first));
            const uint64_t grp = __ballot(bin == lb);
            if (lane == first) atomicAdd(&h[col * hw + (lb >> 1)], uint32_t(__popcll(grp)) << ((lb & 1u) * 16u));
            if (grp != act && bin != lb) atomicAdd(&h[col * hw + (bin >> 1)], 1u << ((bin & 1u) * 16u));
          } else {
            // a sample counts for a rank when its found bits (>= fsh, < 32) are the rank's
            const uint32_t hk = k >> fsh[col];
            bool hit = false;
#pragma unroll
            for (int q = 0; q < kLongRanks; ++q)
              if ((cmask[col] >> q) & 1u)
                if (hk == pre[col][q]) {
                  atomicAdd(&h[(col * kLongRanks + q) * 128 + (bin >> 1)], 1u << ((bin & 1u) * 16u));
                  hit = true;
                }
            if constexpr (PASS == 2) {
              // compaction: the wave's hits of this series go to its candidate list with
              // one device atomic (the wave's count), each lane at its rank among them
              if (a.compact) {
                const uint64_t mb = __ballot(hit);
                if (mb) {
                  const int leader = __builtin_ctzll(mb);
                  uint32_t base = 0;
                  if (lane == leader) base = atomicAdd(&sh_.ccount[col], uint32_t(__popcll(mb)));  // LDS
                  base = uint32_t(__builtin_amdgcn_readlane(int(base), leader));
                  if (hit) {
                    const uint32_t off =
                        __builtin_amdgcn_mbcnt_hi(uint32_t(mb >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mb), 0u));
                    a.cand[size_t(V.sb + col) * a.cand_cap + size_t(c) * V.chunk_rows + base + off] = k;
                  }
                }
              }
            }
          }
        }
      }
    }
    }  // passes 0-3
    if constexpr (PASS == 0 || PASS == kPassBrk) {
      if constexpr (INNER_FLUSH) {
        flush();  // the iteration's last group
      } else if (++git == UG / U) {
        git = 0;
        flush();
      }
    }
    if (inext < rows) {
      if constexpr (pf) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int col = 0; col < WM; ++col) v[u][col] = vn[u][col];
      } else {
        load_rows(v, inext);
      }
    }
  }

  if constexpr (PASS == 0 || PASS == kPassBrk) {
    if (git) flush();  // a group the chunk's end cut short (its missing rows were NaN)
    // per-chunk partials: wave butterflies, then the 4 waves in a fixed order
#pragma unroll
    for (int col = 0; col < WM; ++col) {
      if (uint32_t(col) < w && ((colmask >> col) & 1u)) {
        double s = sum[col];
        uint32_t cn = cnt[col], lo = mn[col], hi = mx[col], ox = orx[col];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          s += __shfl_xor(s, off);
          cn += __shfl_xor(cn, off);
          lo = min(lo, uint32_t(__shfl_xor(int(lo), off)));
          hi = max(hi, uint32_t(__shfl_xor(int(hi), off)));
          ox |= uint32_t(__shfl_xor(int(ox), off));
        }
        if (lane == 0) {
          sh_.rsum[wave][col] = s;
          sh_.rcnt[wave][col] = cn;
          sh_.rmin[wave][col] = lo;
          sh_.rmax[wave][col] = hi;
          sh_.ror[wave][col] = ox;
        }
        if constexpr (PASS == kPassBrk) {
#pragma unroll
          for (int q = 0; q < kBrkQ; ++q) {
            uint32_t l = lt[col][q];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) l += uint32_t(__shfl_xor(int(l), off));
            if (lane == 0) sh_.rlt[wave][col * kBrkQ + q] = l;
            if constexpr (EQREG) {
              // lo | hi << 16 halves: a chunk holds < 2^16 rows, so neither half carries
              uint32_t e = eqr[col][q];
#pragma unroll
              for (int off = 32; off >= 1; off >>= 1) e += uint32_t(__shfl_xor(int(e), off));
              if (lane == 0) atomicAdd(&sh_.beq[col * kBrkQ + q], e);  // LDS: the 4 waves
            }
          }
        }
      }
    }
  }
}

// Pass 0's prediction of the key bits that vary over ring r's segment (threads t < w
// of the workgroup, one series each; LDS arrays of kSegCols): the previous refresh's
// exact min / max / lowest varying bit and the <= kPredMaxNew rows that entered since
// (0 / ~0 / 0 - no prediction - otherwise), and the newest sample's key as the reference
// of orx. Ends with a barrier.
__device__ inline void lw_predict(const LwArgs& a, uint32_t r, const float* seg, uint32_t stride, uint32_t w,
                                  uint32_t sb, uint32_t* pmin, uint32_t* pmax, uint32_t* plo, uint32_t* plx,
                                  uint32_t* dref) {
  const int t = threadIdx.x;
  const uint64_t head = a.params->head[r], prev = a.params->prev_head[r];
  const uint32_t n = a.params->n[r];
  const bool pred = prev != 0 && head >= prev && head - prev <= kPredMaxNew;
  if (uint32_t(t) < w) {
    const LwSel& sl = a.sel[sb + t];
    pmin[t] = pred ? sl.minkey : 0u;
    pmax[t] = pred ? sl.maxkey : 0xFFFFFFFFu;
    plo[t] = pred ? sl.lo : 0u;  // the previous window's lowest varying bit
    plx[t] = 0;
    // orx's reference: the newest sample (a window member: orx is then exact)
    const float x = n ? seg[((head - 1) & uint64_t(a.mask)) * stride + t] : __builtin_nanf("");
    dref[t] = isnan(x) ? 0u : fkey(x);
  }
  __syncthreads();
  if (pred && uint32_t(t) < uint32_t(head - prev)) {
    const float* p = seg + ((prev + uint32_t(t)) & uint64_t(a.mask)) * stride;
    for (uint32_t col = 0; col < w; ++col) {
      const float x = p[col];
      if (!isnan(x)) {
        const uint32_t k = fkey(x);
        atomicMin(&pmin[col], k);
        atomicMax(&pmax[col], k);
        atomicOr(&plx[col], k ^ a.sel[sb + col].minkey);  // vs a previous member
      }
    }
  }
  __syncthreads();
}

// PF: 0 = no prefetch (U = 4 rows per thread for 8-series segments, 8 for <= 4), 1 =
// prefetch with the same U (two register buffers: fewer waves fit), 2 = prefetch with
// half the rows per buffer (the registers of PF 0)
template <int PASS, int PF>
__device__ __forceinline__ void lw_pass_body(const LwArgs& a) {
  // LDS histogram words per series (pass B keeps no histogram)
  constexpr uint32_t HW = PASS == 0 ? kB0 / 2 : (PASS == kPassBrk ? 0u : kLongRanks * 128);
  static_assert(kLongChunkRowsMax < 65536, "16-bit LDS bins");
  extern __shared__ uint32_t h[];
  __shared__ uint32_t pre[kSegCols * kLongRanks];
  __shared__ uint32_t dshift[kSegCols], dwidth[kSegCols], dref[kSegCols];
  __shared__ uint32_t pmin[kSegCols], pmax[kSegCols], plx[kSegCols], plo[kSegCols];
  __shared__ uint32_t live, maxdw;
  __shared__ uint32_t ccount[kSegCols];
  __shared__ double rsum[NT / 64][kSegCols];
  __shared__ uint32_t rcnt[NT / 64][kSegCols], rmin[NT / 64][kSegCols], rmax[NT / 64][kSegCols], ror[NT / 64][kSegCols];
  __shared__ uint32_t bcnt[kSegCols * kBrkQ], beq[kSegCols * kBrkQ], rlt[NT / 64][kSegCols * kBrkQ];

  uint32_t gi = 0, c = 0, cs1 = 0;
  bool split = false;  // column-split pass B: this workgroup streams column cs1 of the segment only
  if (PASS == kPassBrk && a.nwork) {  // incremental pass B: the host's list of (segment, chunk)
    const uint32_t e = a.work[blockIdx.x];
    c = e & 0xFFFFFu;
    if (a.colsplit) {
      gi = e >> 23;
      cs1 = (e >> 20) & 7u;
      split = true;
    } else {
      gi = e >> 20;
    }
  } else {
    for (uint32_t i = 1; i < a.num_segs; ++i)  // the segment whose workgroup range holds this one
      if (blockIdx.x >= a.segs[i].wg0) gi = i;
    c = blockIdx.x - a.segs[gi].wg0;
  }
  const LwSeg G = a.segs[gi];
  const uint32_t r = G.ring;
  const LwRing R = a.rings[r];
  const uint32_t col0 = G.col0 + cs1;                 // the first column this workgroup streams
  const uint32_t w = split ? 1u : G.ncols;            // series it streams
  const uint32_t sb = R.first_series + col0;          // its first series
  const float* seg = R.dev + col0;                    // row i: seg + i * R.width
  const int t = threadIdx.x;

  if constexpr (PASS == 0) {
    if (t == 0) {
      maxdw = 1;
      live = 0;  // columns to stream: those scan B did not resolve
    }
    __syncthreads();
    if (uint32_t(t) < w && !(a.brk_on && a.sel[sb + t].done)) atomicOr(&live, 1u << t);
    __syncthreads();
    if (!live) return;  // scan B resolved every series of the segment (uniform): no prediction either
    if (a.node_n == 0) {
      lw_predict(a, r, seg, R.width, w, sb, pmin, pmax, plo, plx, dref);
    } else {
      // node mode: every rank combines the all-gathered predictions in rank order, so
      // every rank picks the same digit. The node window lies inside the union of the
      // ranks' predicted sets: min / max over them; the varying bits are each rank's
      // plus those where the ranks' reference keys differ, and the common reference
      // key is the first rank's that holds samples (a node-window member)
      if (uint32_t(t) < w) {
        uint32_t mn = 0xFFFFFFFFu, mx = 0u, lo = 32u, ref = 0u;
        bool any = false;
        for (uint32_t q = 0; q < a.node_n; ++q) {
          const LwPred p = a.pred_all[size_t(q) * a.num_series + sb + t];
          mn = min(mn, p.pmin);
          mx = max(mx, p.pmax);
          lo = min(lo, p.lo);
          if (p.has) {
            if (!any) {
              ref = p.ref;
              any = true;
            } else if (p.ref != ref) {
              lo = min(lo, uint32_t(__builtin_ctz(p.ref ^ ref)));
            }
          }
        }
        pmin[t] = mn;
        pmax[t] = mx;
        plo[t] = lo;
        plx[t] = 0;
        dref[t] = ref;
      }
      __syncthreads();
    }
    if (uint32_t(t) < w) {
      const uint32_t d = pmin[t] ^ pmax[t];
      const uint32_t top = d ? 31u - uint32_t(__builtin_clz(d)) : 0u;
      // the digit width: 10 bits when that saves a pass over 8 (the predicted span, down
      // to the predicted lowest varying bit), else 8 - the top byte of mixed-sign data
      // falls into few bins (one atomic per wave), 10 bits would not
      const uint32_t lo = min(plo[t], plx[t] ? uint32_t(__builtin_ctz(plx[t])) : 32u);
      const uint32_t span = top >= lo ? top - lo + 1 : 1u;
      const auto passes = [span](uint32_t dw) { return span > dw ? (span - dw + 7) / 8 : 0u; };
      const uint32_t dw = passes(kD0) < passes(8) ? uint32_t(kD0) : 8u;
      dwidth[t] = dw;
      atomicMax(&maxdw, dw);
      dshift[t] = top >= dw - 1 ? top - (dw - 1) : 0u;
      if (c == 0) {  // every workgroup of the ring computes the same: chunk 0 tells scan 0
        a.dig0[3 * (sb + t)] = dshift[t];
        a.dig0[3 * (sb + t) + 1] = dref[t];
        a.dig0[3 * (sb + t) + 2] = dw;
      }
    }
  } else if constexpr (PASS == kPassBrk) {
    if (t == 0) live = 0;
    // scan B decides with a copy of every series' brackets (it writes the next ones into
    // brk while its other workgroups still read): the grid's first workgroup makes it, in
    // the flat grid and in the incremental work list alike
    if (blockIdx.x == 0)
      for (uint32_t i = t; i < a.num_series; i += NT) a.brk_used[i] = a.brk[i];
    __syncthreads();
    if (uint32_t(t) < w && a.brk[sb + t].valid) atomicOr(&live, 1u << t);
    if (uint32_t(t) < kSegCols * kBrkQ) bcnt[t] = beq[t] = 0;
    __syncthreads();
    if (!live) return;  // no series of the segment has brackets this refresh (uniform)
    if (uint32_t(t) < w) {
      // orx's reference: the newest sample (a window member), as pass 0's
      const uint32_t n = a.params->n[r];
      const float x = n ? seg[((a.params->head[r] - 1) & uint64_t(a.mask)) * R.width + t] : __builtin_nanf("");
      dref[t] = isnan(x) ? 0u : fkey(x);
    }
    __syncthreads();
  } else {
    if (t == 0) live = 0;
    __syncthreads();
    if (uint32_t(t) < w) {
      const LwSel& sl = a.sel[sb + t];
      dshift[t] = sl.shift;
      dwidth[t] = sl.width;
      if (sl.width) atomicOr(&live, 1u);
    }
    for (uint32_t i = t; i < w * kLongRanks; i += NT) pre[i] = a.sel[sb + i / kLongRanks].prefix[i % kLongRanks];
    __syncthreads();
    if (!live) return;  // every series of the ring is resolved: nothing to stream
  }
  if constexpr (PASS == 0) __syncthreads();  // maxdw
  // LDS words per series: pass 0 sized by the ring's widest digit (the launch reserves 10 bits)
  const uint32_t hw = PASS == 0 ? (1u << maxdw) / 2 : HW;
  // pass 0 with 8-bit digits (the top byte: mixed signs, or no prediction) puts most
  // samples of a series into one or two bins, and the 4 waves' atomics then queue on the
  // same LDS words: with wave_priv each wave counts into its own copy (4 x 8-bit copies
  // fit the 10-bit reservation), summed word-wise in the merge (a bin's halves stay
  // below 2^16 over all copies: <= kLongChunkRows samples per workgroup)
  // wave_priv 2: a copy per half wave (32 lanes), the copies 16 banks apart - half the
  // lanes that share a bin per atomic (launch reserves 8 x (w x 128 + 16) words)
  const uint32_t lvl = (PASS == 0 && maxdw == 8) ? a.wave_priv : 0u;
  const uint32_t copies = lvl == 2 ? 2 * (NT / 64) : (lvl == 1 ? NT / 64 : 1u);
  const uint32_t cs = w * hw + (lvl == 2 ? 16u : 0u);  // words per copy
  for (uint32_t i = t; i < copies * cs; i += NT) h[i] = 0;
  if (uint32_t(t) < kSegCols) ccount[t] = 0;
  __syncthreads();

  const uint32_t colmask = (PASS == 0 || PASS == kPassBrk) ? live : 0xFFFFFFFFu;
  const LwShared sh_{pre, dshift, dwidth, dref, rsum, rcnt, rmin, rmax, ror, ccount, colmask, bcnt, beq, rlt};
  const LwView V{seg,
                 R.width,
                 R.chunk_rows,
                 w,
                 !split && ((R.width | col0) & 3u) == 0,
                 sb,
                 a.bcand ? a.bcand + R.boff + size_t(col0) * R.bstride : nullptr,
                 R.bstride,
                 R.qcap,
                 a.brk,
                 (1u << kBrkQ) - 1u,
                 nullptr,
                 false,
                 nullptr};
  uint32_t* hmine = h + (lvl == 2 ? uint32_t(t >> 5) : (lvl == 1 ? uint32_t(t >> 6) : 0u)) * cs;
  // rows per thread per buffer, 8-series segments (pass B: 2 - its bracket counters take
  // the registers of the other rows)
  constexpr int UN = (PF == 2 || PASS == kPassBrk) ? 2 : 4;
  if constexpr (PASS == kPassBrk) {
    if (split) {  // one column, in its segment's sum groups
      // (with the next rows' loads in flight: a lone workgroup per chunk is latency-bound)
      // 32 rows per thread per iteration, the next 32 in flight: a chunk of 24576 rows is 3
      // iterations, ~3 memory latencies instead of 24
      if (G.ncols <= 4) pass_chunk<PASS, 1, 32, true, 8>(a, V, r, c, hmine, hw, sh_);
      else pass_chunk<PASS, 1, 32, true, 4>(a, V, r, c, hmine, hw, sh_);
    } else if (w <= 4) {
      pass_chunk<PASS, 4, 2 * UN, PF != 0>(a, V, r, c, hmine, hw, sh_);
    } else {
      pass_chunk<PASS, kSegCols, UN, PF != 0>(a, V, r, c, hmine, hw, sh_);
    }
  } else {
    if (w <= 4) pass_chunk<PASS, 4, 2 * UN, PF != 0>(a, V, r, c, hmine, hw, sh_);
    else pass_chunk<PASS, kSegCols, UN, PF != 0>(a, V, r, c, hmine, hw, sh_);
  }
  __syncthreads();
  if (copies > 1) {  // fold the wave copies into copy 0
    for (uint32_t i = t; i < w * hw; i += NT) {
      uint32_t x = h[i];
      for (uint32_t k = 1; k < copies; ++k) x += h[k * cs + i];
      h[i] = x;
    }
    __syncthreads();
  }
  if constexpr (PASS == 2) {  // the chunk's candidate count per series (pass 3 reads its slab)
    if (a.compact && uint32_t(t) < w) a.cand_n[size_t(sb + t) * a.max_chunks + c] = ccount[t];
  }
  if constexpr (PASS == 0 || PASS == kPassBrk) {
    if (uint32_t(t) < w && ((colmask >> t) & 1u)) {
      LwPartial pp{0.0, 0, 0xFFFFFFFFu, 0, 0, dref[t], 0};  // every sample's orx is relative to dref
      for (int wv = 0; wv < NT / 64; ++wv) {
        pp.sum += rsum[wv][t];
        pp.cnt += rcnt[wv][t];
        pp.minkey = min(pp.minkey, rmin[wv][t]);
        pp.maxkey = max(pp.maxkey, rmax[wv][t]);
        pp.orx |= ror[wv][t];
      }
      a.part[size_t(sb + t) * a.max_chunks + c] = pp;
      if constexpr (PASS == kPassBrk) {
        LwBrkPart bp{};
        for (int q = 0; q < kBrkQ; ++q) {
          bp.mid[q] = bcnt[t * kBrkQ + q];
          bp.eq[q] = beq[t * kBrkQ + q];
          for (int wv = 0; wv < NT / 64; ++wv) bp.lt[q] += rlt[wv][t * kBrkQ + q];
        }
        a.bpart[size_t(sb + t) * a.max_chunks + c] = bp;
      }
    }
  }
  if constexpr (PASS != kPassBrk) {  // pass B keeps no histogram
    // merge the non-zero bins: one device-scope atomic each (kernel boundary publishes)
    constexpr uint32_t GB = PASS == 0 ? kB0 : kLongRanks * 256;  // global bins per series
    uint32_t* g = (PASS == 0 ? a.hist0 : a.histk) + size_t(sb) * GB;
    for (uint32_t i = t; i < w * hw; i += NT) {
      const uint32_t x = h[i];
      const uint32_t b = PASS == 0 ? (i / hw) * GB + 2 * (i % hw) : 2 * i;  // pass 0: series, bin
      if (x & 0xFFFFu) atomicAdd(&g[b], x & 0xFFFFu);
      if (x >> 16) atomicAdd(&g[b + 1], x >> 16);
    }
  }
}

}  // namespace
}  // namespace rocmdash
