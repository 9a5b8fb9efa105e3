// Long-window bracket mode (long_window.h): pass B, scan B (plain, fused, and the node's
// two halves), the report, and the ingest kernel that stages a small refresh.
//
// Bracket mode (lw_pass_brk, lw_scan_brk). A window changes by the few rows that
// entered and left since the previous refresh, so each percentile moves by at most a few
// ranks: the previous refresh's percentile keys, widened by an adaptive half-width, bracket
// the new ones. One streaming pass counts, per percentile q, the samples below the
// bracket (lt), ON its bounds (counted, never kept) and strictly inside it (kept); if both
// sorted positions of every percentile fall inside their brackets (lt <= pos < lt + in),
// the percentiles are the lower bound, the upper bound or order statistics of the kept
// keys - a select over ~kBrkTarget keys in LDS instead of 2-3 more streams of the window.
// Otherwise (the first refresh, a jump in the data, a bracket that overflowed) the series
// takes the exact radix chain in the same refresh. The half-width adapts so that a bracket
// holds ~kBrkTarget samples; a bracket on tied values (integer telemetry, a percentile
// between two readings) is exactly those keys and stores nothing - its ties are counts.
// Known limit: each (chunk, bracket) keeps at most qcap keys, so a series whose bracket
// samples are consecutive rows (a monotone ramp) overflows one chunk's slab and takes the
// radix chain every refresh (exact, at the chain's cost); the service's series are gauges
// and rates, not ramps.

#include "long_window_pass.h"
#include "window_stats.h"

namespace rocmdash {
namespace {

// pass B (bracket counts): 4 waves per SIMD, as pass 0 - its per-lane bracket counters
// would otherwise take it to 3
__global__ __launch_bounds__(NT, 4) void lw_pass_brk(const LwArgs a) {
  lw_pass_body<kPassBrk, 0>(a);
}

// The keys at sorted positions ra <= rb among the n keys of a bracket [lo, lo + 2^bits)
// in LDS: an LDS radix select on key - lo, kSelBits per pass from the top (two prefixes
// while the ranks' digits agree, one histogram each once they differ).
__device__ inline void lds_select2(const uint32_t* keys, uint32_t n, uint32_t lo, uint32_t bits, uint32_t ra,
                                   uint32_t rb, uint32_t* hist, uint32_t* tmp, uint32_t* found, uint32_t& ka,
                                   uint32_t& kb) {
  constexpr uint32_t NB = 1u << kSelBits, BPT = NB / NT;
  const int t = threadIdx.x;
  uint32_t pa = 0, pb = 0;  // found bits of key - lo (above `shift`)
  uint32_t shift = bits;
  while (shift > 0) {
    const uint32_t wd = min(kSelBits, shift), ns = shift - wd;
    for (uint32_t i = t; i < 2 * NB; i += NT) hist[i] = 0;
    __syncthreads();
    for (uint32_t i = t; i < n; i += NT) {
      const uint32_t d = keys[i] - lo;
      const uint32_t hi = shift >= 32 ? 0u : d >> shift;
      const uint32_t dig = (d >> ns) & ((1u << wd) - 1u);
      if (hi == pa) atomicAdd(&hist[dig], 1u);
      if (pb != pa && hi == pb) atomicAdd(&hist[NB + dig], 1u);
    }
    __syncthreads();
    for (int k = 0; k < 2; ++k) {
      const uint32_t* H = hist + (k == 1 && pb != pa ? NB : 0u);
      const uint32_t rq = k == 0 ? ra : rb;
      uint32_t v[BPT], tot = 0;
#pragma unroll
      for (uint32_t j = 0; j < BPT; ++j) {
        v[j] = H[t * BPT + j];
        tot += v[j];
      }
      uint32_t excl, incl, all;
      block_scan_total(tot, tmp, excl, incl, all);
      if (tot && excl <= rq && rq < incl) {
        for (uint32_t j = 0; j < BPT; ++j) {
          if (v[j] && excl <= rq && rq < excl + v[j]) {
            found[2 * k] = t * BPT + j;
            found[2 * k + 1] = rq - excl;
          }
          excl += v[j];
        }
      }
      __syncthreads();
    }
    pa = (pa << wd) | found[0];
    ra = found[1];
    pb = (pb << wd) | found[2];
    rb = found[3];
    __syncthreads();  // found reusable
    shift = ns;
  }
  ka = lo + pa;
  kb = lo + pb;
}

// scan B: one workgroup per (series, bracket q). Each reduces pass B's partials and the
// bracket counts of all three brackets (the same decision in the three workgroups): if
// every percentile's lo and hi positions fall inside their brackets (and no slab
// overflowed), workgroup q selects its two keys among bracket q's kept keys and writes
// percentile q; workgroup 0 writes min / max / mean / count / last and marks the series
// done - the radix chain then skips it; else it is left to the radix chain (done = 0).
// The brackets pass B used come from brk_used (pass B's copy); the next refresh's go to
// brk.
// scan B's phase clocks (LongWindowSet::set_phase_clocks): workgroup (s, q) thread 0
// writes the shader clock at phase k - a vector store to device memory
__device__ inline void lw_clock(const LwArgs& a, uint32_t s, int q, int k) {
  if (a.dbg && threadIdx.x == 0) a.dbg[(size_t(s) * kBrkQ + q) * 8 + k] = __builtin_readcyclecounter();
}

// The rest of scan B, shared by its local (lw_scan_brk) and node (lw_node_brk_select)
// forms once the bracket counts are known: the hit decision, this workgroup's select (the
// ranks on a bound are the bound; the others among the kept keys, `gather` fills LDS with
// bracket q's), the next brackets and the outputs.
struct LwBrkCounts {
  uint32_t lt[kBrkQ];   // below
  uint32_t mid[kBrkQ];  // strictly inside (kept)
  uint32_t elo[kBrkQ];  // on lo
  uint32_t ehi[kBrkQ];  // on hi (hi != lo)
  uint32_t ovf;         // bracket bits whose kept keys did not all fit
};
template <class Gather>
__device__ inline void lw_brk_resolve(const LwArgs& a, uint32_t s, int q, const LwBrk& b, const LwPartial& tot,
                                      const LwBrkCounts& C, uint64_t entered, uint32_t r, uint32_t col,
                                      uint32_t* keys, uint32_t* hist, uint32_t* tmp, uint32_t* found,
                                      uint32_t (*red)[NT / 64], Gather gather) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const LwRing R = a.rings[r];
  const uint32_t nv = tot.cnt;
  uint32_t pos[kLongRanks];
  double frac[3];
  lw_positions(nv, a.params->pct, pos, frac);
  bool hit = nv > 0;
  // this workgroup's bracket (selected by unrolled compares: no dynamic register indexing)
  uint32_t lq = 0, hq = 0, dq = 0, ltq = 0, inq = 0, midq = 0, eloq = 0, p0 = 0, p1 = 0;
  bool ovq = false;
  double fq = 0.0;
#pragma unroll
  for (int k = 0; k < kBrkQ; ++k) {
    const uint32_t in = C.mid[k] + C.elo[k] + C.ehi[k];
    const bool ov = ((C.ovf >> k) & 1u) || C.mid[k] > kBrkCap;
    hit = hit && !ov && C.lt[k] <= pos[2 * k] && pos[2 * k + 1] < C.lt[k] + in;
    if (k == q) {
      lq = b.lo[k];
      hq = b.hi[k];
      dq = b.delta[k];
      ltq = C.lt[k];
      inq = in;
      midq = C.mid[k];
      eloq = C.elo[k];
      ovq = ov;
      p0 = pos[2 * k];
      p1 = pos[2 * k + 1];
      fq = frac[k];
    }
  }
  LwBrk* nb = a.brk + s;  // the next refresh's brackets (this workgroup writes field q)
  if (!hit) {  // the radix chain resolves the series; its scan 3 sets the next brackets
    if (t == 0) {
      nb->cin[q] = inq;
      // more kept keys than fit: read as ties between the percentile's keys (telemetry
      // readings) - the next bracket is exactly the keys the chain finds, their ties then
      // counted on its bounds, not kept. Continuous data that overflowed (rare: the first
      // estimate aims low) gets a value half-width back a refresh later (few inside)
      if (ovq) {
        // put the value half-width the normal rule would take aside: if the exact bracket
        // then holds few samples (not ties), the bracket resumes from it
        const float dv = __uint_as_float(dq);
        if (dv > 0.f)
          nb->dsave[q] = __float_as_uint(float(double(dv) * fmin(8.0, double(lw_brk_target(a, nv)) /
                                                                        double(max(inq, 1u)))));
        nb->delta[q] = 0u;
        nb->nounion[q] = 1u;
      }
      if (q == 0) {
        a.sel[s].done = 0;
        nb->refreshes = b.refreshes + 1;
      }
    }
    return;
  }
  const uint32_t target = lw_brk_target(a, nv);
  // every percentile inside its bracket: ranks on the lower bound are lo, past the kept
  // keys hi, between them a select among the kept keys
  const uint32_t r0 = p0 - ltq, r1 = p1 - ltq;
  const bool m0 = r0 >= eloq && r0 < eloq + midq, m1 = r1 >= eloq && r1 < eloq + midq;
  uint32_t k0 = r0 < eloq ? lq : hq, k1 = r1 < eloq ? lq : hq;
  lw_clock(a, s, q, 2);
  if (m0 || m1) {  // uniform
    gather(keys);  // bracket q's kept keys into LDS (midq of them)
    __syncthreads();
    lw_clock(a, s, q, 3);
    const uint32_t span = hq - lq;
    const uint32_t bits = 32u - uint32_t(__builtin_clz(span));
    uint32_t s0 = 0, s1 = 0;
    lds_select2(keys, midq, lq, bits, m0 ? r0 - eloq : r1 - eloq, m1 ? r1 - eloq : r0 - eloq, hist, tmp, found, s0,
                s1);
    if (m0) k0 = s0;
    if (m1) k1 = s1;
    lw_clock(a, s, q, 4);
  }
  // ties: every kept key is the percentile's own (integer telemetry) - an exact-key
  // bracket then holds the rank with no keys to keep (red[0] / red[1]: key min / max)
  bool ties = false;
  if (midq && k0 == k1 && m0 && m1) {  // uniform
    uint32_t kmn = 0xFFFFFFFFu, kmx = 0;
    for (uint32_t i = t; i < midq; i += NT) {
      kmn = min(kmn, keys[i]);
      kmx = max(kmx, keys[i]);
    }
    for (int off = 32; off >= 1; off >>= 1) {
      kmn = min(kmn, uint32_t(__shfl_xor(int(kmn), off)));
      kmx = max(kmx, uint32_t(__shfl_xor(int(kmx), off)));
    }
    if (lane == 0) {
      red[0][wave] = kmn;
      red[1][wave] = kmx;
    }
    __syncthreads();
    if (t == 0) {
      for (int wv = 1; wv < NT / 64; ++wv) {
        red[0][0] = min(red[0][0], red[0][wv]);
        red[1][0] = max(red[1][0], red[1][wv]);
      }
    }
    __syncthreads();
    ties = red[0][0] == k0 && red[1][0] == k0;
  }
  if (t == 0) {
    uint32_t nlo = lq, nhi = hq, nd = dq;
    // incremental mode: the bracket stays put while both positions sit well inside it and
    // it holds a sane number of samples (an exact-key bracket: any number - its ties are
    // counted, not kept) - its chunks' counts then stay valid and the next pass B streams
    // only the chunks new rows landed in; otherwise (and always without incr) it is
    // re-centred on the keys just found
    bool keep = false;
    if (a.incr) {
      // the margin: twice the rows that entered (how far a position can move by the next
      // refresh at this rate), at most an eighth of the bracket. Node brackets: the rows
      // that entered the whole node (the same on every rank - the brackets must stay so)
      const uint64_t ent = entered == ~uint64_t(0) ? uint64_t(inq) : entered;
      const uint32_t m = max(8u, uint32_t(min<uint64_t>(inq / 8, 2 * ent)));
      const bool exact = dq == 0u;
      const bool inside = p0 >= ltq + m && p1 + m < ltq + inq;
      const bool sized = exact || (inq <= 2 * target && 4 * inq >= target);  // the select costs what it keeps
      keep = inside && sized && !ties;
    }
    if (ties) {  // -> an exact-key bracket on the tied value
      nlo = nhi = k0;
      nd = 0u;
      if (a.bchg) a.bchg[s] = 1u;
    } else if (!keep) {
      lw_next_bracket(nd, inq, nlo, nhi, k0, k1, lw_brk_est(tot.minkey, tot.maxkey, nv, target), true, target, true,
                      &nb->dsave[q]);
      if (a.bchg && (nlo != lq || nhi != hq)) a.bchg[s] = 1u;  // its chunks' counts are stale now
    }
    nb->lo[q] = nlo;
    nb->hi[q] = nhi;
    nb->delta[q] = nd;
    nb->cin[q] = inq;
    const double x0 = kfloat(k0), x1 = kfloat(k1);
    a.out[size_t(s) * STAT_NUM + STAT_P0 + q] = float(fq >= 0.5 ? x1 - (x1 - x0) * (1.0 - fq) : x0 + (x1 - x0) * fq);
  }
  lw_clock(a, s, q, 5);
  if (q != 0) return;
  const uint32_t lov = tot.orx ? uint32_t(__builtin_ctz(tot.orx)) : 32u;
  if (t == 0) {
    LwSel S = a.sel[s];
    S.nv = nv;
    S.minkey = tot.minkey;
    S.maxkey = tot.maxkey;
    S.sum = tot.sum;
    S.lo = lov;
    S.width = 0;
    S.done = 1;
    a.sel[s] = S;
    const uint32_t want = a.incr ? (nv ? 1u : 0u) : lw_brk_wanted(nv, tot.minkey, tot.maxkey, lov);
    if (a.bchg && want != b.valid) a.bchg[s] = 1u;
    nb->valid = want;
    nb->hit = 1;
    nb->hits = b.hits + 1;
    nb->refreshes = b.refreshes + 1;
    if (a.hflags) a.hflags[s] = want;
  }
  if (t < STAT_NUM && (t < STAT_P0 || t >= STAT_P0 + kBrkQ)) {
    const uint64_t head = a.params->head[r];
    const uint32_t n = a.params->n[r];
    float o = __builtin_nanf("");
    if (t == STAT_COUNT) {
      o = float(nv);
    } else if (t == STAT_LAST) {  // node brackets: no node-wide newest sample (NaN)
      if (n && !a.node_brk) o = R.dev[((head - 1) & uint64_t(a.mask)) * R.width + col];
    } else if (t == STAT_MIN) {
      o = kfloat(tot.minkey);
    } else if (t == STAT_MAX) {
      o = kfloat(tot.maxkey);
    } else if (t == STAT_MEAN) {
      o = float(tot.sum / double(nv));
    }
    a.out[size_t(s) * STAT_NUM + t] = o;
  }
}

// Pass B's per-chunk bracket counts of series s, summed over the ring's chunks (every
// thread gets the totals). ovf: a chunk kept fewer keys than were strictly inside.
// tot != nullptr (scan B): the chunks' partials combined in the same loop (one memory round
// trip for both; the partial's reduction order is reduce_partials')
__device__ inline LwBrkCounts lw_brk_counts(const LwArgs& a, uint32_t s, const LwRing& R, const LwBrk& b,
                                            uint32_t (*red)[NT / 64], LwPartial* tot = nullptr,
                                            double* dsum = nullptr, uint32_t* dcnt = nullptr, uint32_t* dmin = nullptr,
                                            uint32_t* dmax = nullptr, uint32_t* dor = nullptr, uint32_t* drf = nullptr) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t v[4 * kBrkQ + 1];
#pragma unroll
  for (int i = 0; i < 4 * kBrkQ + 1; ++i) v[i] = 0;
  double sm = 0.0;
  uint32_t cn = 0, lo = 0xFFFFFFFFu, hi = 0, ox = 0, rf = 0;
  if (b.valid) {
    // unrolled: a thread's chunks' loads in flight together (scan B's first phase was one
    // memory round trip per 256 chunks)
#pragma unroll 8
    for (uint32_t i = t; i < R.nchunks; i += NT) {
      if (tot) {
        const LwPartial pp = a.part[size_t(s) * a.max_chunks + i];
        lw_combine(sm, cn, lo, hi, ox, rf, pp.sum, pp.cnt, pp.minkey, pp.maxkey, pp.orx, pp.ref);
      }
      const LwBrkPart bp = a.bpart[size_t(s) * a.max_chunks + i];
#pragma unroll
      for (int k = 0; k < kBrkQ; ++k) {
        v[k] += bp.lt[k];
        v[kBrkQ + k] += bp.mid[k];
        v[2 * kBrkQ + k] += eq_lo(bp.eq[k]);
        v[3 * kBrkQ + k] += eq_hi(bp.eq[k]);
        if (bp.mid[k] > R.qcap) v[4 * kBrkQ] |= 1u << k;
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 4 * kBrkQ; ++i) v[i] += uint32_t(__shfl_xor(int(v[i]), off));
    v[4 * kBrkQ] |= uint32_t(__shfl_xor(int(v[4 * kBrkQ]), off));
  }
  __syncthreads();  // red may still be read by the caller's previous phase
  if (lane == 0)
    for (int i = 0; i < 4 * kBrkQ + 1; ++i) red[i][wave] = v[i];
  __syncthreads();
  LwBrkCounts C{};
  for (int wv = 0; wv < NT / 64; ++wv) {
    for (int k = 0; k < kBrkQ; ++k) {
      C.lt[k] += red[k][wv];
      C.mid[k] += red[kBrkQ + k][wv];
      C.elo[k] += red[2 * kBrkQ + k][wv];
      C.ehi[k] += red[3 * kBrkQ + k][wv];
    }
    C.ovf |= red[4 * kBrkQ][wv];
  }
  __syncthreads();  // red reusable
  if (tot) *tot = block_reduce_partial(sm, cn, lo, hi, ox, rf, dsum, dcnt, dmin, dmax, dor, drf);
  return C;
}

// Bracket q's kept keys of series s (every chunk's slab, chunk order) into dst. Thread t
// owns a contiguous run of chunks (<= kGatherRun of them): their counts are loaded at once,
// one block scan places the runs, then the first kGatherKeys keys of each of its chunks are
// loaded into registers with independent (predicated) loads - one memory round trip for
// the whole run - and stored; a chunk with more keys (rare: a bracket holds ~2048 samples
// over thousands of chunks) copies the rest in order.
constexpr uint32_t kGatherRun = 16, kGatherKeys = 4;
template <bool BATCH, class Dst>
__device__ inline void lw_gather_slabs(const LwArgs& a, uint32_t s, const LwRing& R, uint32_t col, int q, Dst dst,
                                       uint32_t* tmp) {
  const int t = threadIdx.x;
  const LwBrkPart* bp = a.bpart + size_t(s) * a.max_chunks;
  const uint32_t* slab = a.bcand + R.boff + size_t(col) * R.bstride;
  const uint32_t n = R.nchunks;
  const uint32_t per = (n + NT - 1) / NT;
  const uint32_t c_lo = min(uint32_t(t) * per, n), c_hi = min(c_lo + per, n);
  if (BATCH && per <= kGatherRun) {
    uint32_t m[kGatherRun];
#pragma unroll
    for (uint32_t k = 0; k < kGatherRun; ++k) m[k] = c_lo + k < c_hi ? bp[c_lo + k].mid[q] : 0u;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kGatherRun; ++k) mine += m[k];
    uint32_t excl, incl, total;
    block_scan_total(mine, tmp, excl, incl, total);
    uint32_t v[kGatherRun][kGatherKeys];
#pragma unroll
    for (uint32_t k = 0; k < kGatherRun; ++k) {
      const uint32_t* src = slab + (size_t(c_lo + k) * kBrkQ + q) * R.qcap;
#pragma unroll
      for (uint32_t j = 0; j < kGatherKeys; ++j) v[k][j] = j < m[k] ? src[j] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < kGatherRun; ++k) {
#pragma unroll
      for (uint32_t j = 0; j < kGatherKeys; ++j)
        if (j < m[k]) dst(excl + j, v[k][j]);
      if (m[k] > kGatherKeys) {
        const uint32_t* src = slab + (size_t(c_lo + k) * kBrkQ + q) * R.qcap;
        for (uint32_t j = kGatherKeys; j < m[k]; ++j) dst(excl + j, src[j]);
      }
      excl += m[k];
    }
    return;
  }
  uint32_t mine = 0;
  for (uint32_t c = c_lo; c < c_hi; ++c) mine += bp[c].mid[q];
  uint32_t excl, incl, total;
  block_scan_total(mine, tmp, excl, incl, total);
  for (uint32_t c = c_lo; c < c_hi; ++c) {
    const uint32_t m = bp[c].mid[q];
    const uint32_t* src = slab + (size_t(c) * kBrkQ + q) * R.qcap;
    for (uint32_t j = 0; j < m; ++j) dst(excl + j, src[j]);
    excl += m;
  }
}

__device__ inline void lw_brk_finish(const LwArgs& a);

// Fused pass B (a short work list - the steady state: the 1-2 chunks new rows landed in):
// workgroup (s, q) of scan B streams series s's changed chunks itself, one after another,
// exactly as a column-split pass B workgroup would (the same rows per thread, the same
// segment sum groups: the same partial bits), against the brackets pass B would use
// (brk_used: lw_ingest copied them) - one kernel fewer, and no pass B workgroups to drain.
// The three workgroups of a series write the same partials and bracket counts (identical
// bits: counts do not depend on order), but only bracket q's kept keys (their slab order
// is the workgroup's own), so each reads back exactly what it needs.
__device__ inline void lw_fused_passb(const LwArgs& a, uint32_t s, uint32_t qkeys, uint32_t r, uint32_t col) {
  __shared__ double rsum[NT / 64][kSegCols];
  __shared__ uint32_t rcnt[NT / 64][kSegCols], rmin[NT / 64][kSegCols], rmax[NT / 64][kSegCols],
      ror[NT / 64][kSegCols];
  __shared__ uint32_t bcnt[kSegCols * kBrkQ], beq[kSegCols * kBrkQ], rlt[NT / 64][kSegCols * kBrkQ];
  __shared__ uint32_t dref[kSegCols];
  const int t = threadIdx.x;
  const LwRing R = a.rings[r];
  uint32_t gi = 0;  // the segment holding the series (the work list names segments)
  for (uint32_t i = 0; i < a.num_segs; ++i)
    if (a.segs[i].ring == r && col >= a.segs[i].col0) gi = i;
  const LwSeg G = a.segs[gi];
  const float* seg = R.dev + col;
  // orx's reference, the newest sample (a window member), as pass B's: pass_chunk loads it
  // behind the rows (fused_ref) and leaves its key in dref[0]
  const uint32_t n = a.params->n[r];
  const float* newest = n ? seg + ((a.params->head[r] - 1) & uint64_t(a.mask)) * R.width : nullptr;
  const LwShared sh_{nullptr, nullptr, nullptr, dref, rsum, rcnt, rmin, rmax, ror, nullptr, 1u, bcnt, beq, rlt};
  const LwView V{seg,      R.width, R.chunk_rows, 1u,     false, s,   a.bcand + R.boff + size_t(col) * R.bstride,
                 R.bstride, R.qcap, a.brk_used,  qkeys,   newest, true, dref};
  if (uint32_t(t) < kSegCols * kBrkQ) bcnt[t] = beq[t] = 0;
  __syncthreads();
  for (uint32_t i = 0; i < a.nfused; ++i) {
    const uint32_t e = a.fwork[i];
    if ((e >> 20) != gi) continue;  // uniform
    const uint32_t c = e & 0xFFFFFu;
    if (G.ncols <= 4) pass_chunk<kPassBrk, 1, 32, true, 8>(a, V, r, c, nullptr, 0, sh_);
    else pass_chunk<kPassBrk, 1, 32, true, 4>(a, V, r, c, nullptr, 0, sh_);
    __syncthreads();
    if (t == 0) {  // as lw_pass_body's epilogue: the 4 waves in a fixed order
      LwPartial pp{0.0, 0, 0xFFFFFFFFu, 0, 0, dref[0], 0};
      LwBrkPart bp{};
      for (int wv = 0; wv < NT / 64; ++wv) {
        pp.sum += rsum[wv][0];
        pp.cnt += rcnt[wv][0];
        pp.minkey = min(pp.minkey, rmin[wv][0]);
        pp.maxkey = max(pp.maxkey, rmax[wv][0]);
        pp.orx |= ror[wv][0];
      }
      for (int k = 0; k < kBrkQ; ++k) {
        bp.mid[k] = bcnt[k];
        bp.eq[k] = beq[k];
        bcnt[k] = beq[k] = 0;  // the next chunk's
        for (int wv = 0; wv < NT / 64; ++wv) bp.lt[k] += rlt[wv][k];
      }
      a.part[size_t(s) * a.max_chunks + c] = pp;
      a.bpart[size_t(s) * a.max_chunks + c] = bp;
    }
    __syncthreads();  // the LDS counters and sums are the next chunk's
  }
  // the slab keys and counts written above are this workgroup's own: the barrier (workgroup
  // scope) orders them before its reads - no device-scope fence (an L2 write-back)
  __syncthreads();
}

template <bool FUSED>
__device__ __forceinline__ void lw_scan_brk_body(const LwArgs& a) {
  __shared__ double dsum[NT];
  __shared__ uint32_t dcnt[NT], dmin[NT], dmax[NT], dor[NT], drf[NT];
  __shared__ uint32_t tmp[NT / 64], found[4];
  __shared__ uint32_t red[4 * kBrkQ + 1][NT / 64];
  __shared__ uint32_t keys[kBrkCap];
  __shared__ uint32_t hist[2 << kSelBits];
  const uint32_t s = blockIdx.x;
  const int q = int(blockIdx.y);
  const int t = threadIdx.x;
  const LwBrk b = a.brk_used[s];
  if (!b.valid) {  // no brackets this refresh: the radix chain (its scan 3 sets them)
    if (t == 0 && q == 0) a.sel[s].done = 0;
    return;
  }
  uint32_t r, col;
  series_ring(a, s, r, col);
  const LwRing R = a.rings[r];
  const uint32_t qcap = R.qcap;
  lw_clock(a, s, q, 0);
  if constexpr (FUSED) {
    lw_fused_passb(a, s, 1u << q, r, col);
    lw_clock(a, s, q, 6);
  }
  LwPartial tot;
  const LwBrkCounts C = lw_brk_counts(a, s, R, b, red, &tot, dsum, dcnt, dmin, dmax, dor, drf);
  lw_clock(a, s, q, 1);
  const uint64_t ent = a.params->prev_head[r] ? a.params->head[r] - a.params->prev_head[r] : ~uint64_t(0);
  (void)qcap;
  lw_brk_resolve(a, s, q, b, tot, C, ent, r, col, keys, hist, tmp, found, red, [&](uint32_t* dst) {
    lw_gather_slabs<true>(a, s, R, col, q, [dst](uint32_t i, uint32_t k) { dst[i] = k; }, tmp);
  });
}

// ---- node bracket mode (refresh_node) ------------------------------------------------
// After pass B with the node's brackets: this rank's record of every series - its partials
// over its chunks (in the same order as lw_node_partials: the node mean keeps its bits),
// the bracket counts, and the kept keys of each bracket compacted from the chunk slabs (at
// most kNodeCap; more, or a chunk slab that overflowed, sets the bracket's ovf bit). The
// records are all-gathered: ONE collective carries everything the node's select needs.
__device__ __forceinline__ void lw_node_brk_local_body(const LwArgs& a) {
  __shared__ double dsum[NT];
  __shared__ uint32_t dcnt[NT], dmin[NT], dmax[NT], dor[NT], drf[NT];
  __shared__ uint32_t tmp[NT / 64];
  __shared__ uint32_t red[4 * kBrkQ + 1][NT / 64];
  const uint32_t s = blockIdx.x;
  const int t = threadIdx.x;
  LwNodeHdr* rec = reinterpret_cast<LwNodeHdr*>(a.nbl) + s;
  uint32_t* kept = reinterpret_cast<uint32_t*>(a.nbl + size_t(a.num_series) * sizeof(LwNodeHdr)) +
                   size_t(s) * kBrkQ * a.node_cap;
  const LwBrk b = a.brk_used[s];
  uint32_t r, col;
  series_ring(a, s, r, col);
  const LwRing R = a.rings[r];
  const LwPartial p =
      reduce_partials(a.part + size_t(s) * a.max_chunks, a.max_chunks, 1, dsum, dcnt, dmin, dmax, dor, drf);
  const LwBrkCounts C = lw_brk_counts(a, s, R, b, red);
  uint32_t ovf = C.ovf;
  for (int k = 0; k < kBrkQ; ++k)
    if (C.mid[k] > a.node_cap) ovf |= 1u << k;
  if (!b.valid) ovf = (1u << kBrkQ) - 1u;
  if (t == 0) {
    rec->p = p;
    for (int k = 0; k < kBrkQ; ++k) {
      rec->lt[k] = C.lt[k];
      rec->mid[k] = C.mid[k];
      rec->elo[k] = C.elo[k];
      rec->ehi[k] = C.ehi[k];
    }
    rec->ovf = ovf;
    const uint64_t ph = a.params->prev_head[r];
    rec->ent = ph ? uint32_t(min<uint64_t>(a.params->head[r] - ph, 0xFFFFFFFEull)) : 0xFFFFFFFFu;
  }
  // the kept keys, chunk order; a bracket that overflowed keeps none (it is a miss)
  for (int k = 0; k < kBrkQ; ++k) {
    if (!b.valid || ((ovf >> k) & 1u) || C.mid[k] == 0) continue;  // uniform
    uint32_t* dk = kept + size_t(k) * a.node_cap;
    lw_gather_slabs<false>(a, s, R, col, k, [dk](uint32_t i, uint32_t key) { dk[i] = key; }, tmp);
  }
}

// (A variant streaming short work lists itself, as the local scan B does, was measured in
// rounds 5-6 - 0 to 10 % on a 0.12 ms node refresh, within box noise, profiles/r06/nodewin/ -
// and removed: pass B's own launch stays.)
__global__ __launch_bounds__(NT) void lw_node_brk_local(const LwArgs a) { lw_node_brk_local_body(a); }

// The node's scan B: one workgroup per (series, bracket q). Every rank reduces the
// all-gathered records in rank order - the same node totals, the same decision, the same
// keys selected from the union of the ranks' kept keys - so every rank holds the same
// exact statistics of the node window and the same next brackets.
__device__ __forceinline__ void lw_node_brk_select_body(const LwArgs& a) {
  __shared__ double dsum[NT];
  __shared__ uint32_t dcnt[NT], dmin[NT], dmax[NT], dor[NT], drf[NT];
  __shared__ uint32_t tmp[NT / 64], found[4];
  __shared__ uint32_t red[4 * kBrkQ + 1][NT / 64];
  __shared__ uint32_t keys[kBrkCap];
  __shared__ uint32_t hist[2 << kSelBits];
  const uint32_t s = blockIdx.x;
  const int q = int(blockIdx.y);
  const int t = threadIdx.x;
  const LwBrk b = a.brk_used[s];
  if (!b.valid) {
    if (t == 0 && q == 0) a.sel[s].done = 0;
    return;
  }
  uint32_t r, col;
  series_ring(a, s, r, col);
  // node totals: the partials reduced exactly as the node radix chain's scan 0 reduces them
  // (the same mean bits either way), the counts in rank order
  const size_t block = lw_node_block(a.num_series, a.node_cap);
  auto hdr = [&](uint32_t k) -> const LwNodeHdr& {
    return reinterpret_cast<const LwNodeHdr*>(a.nball + k * block)[s];
  };
  const LwPartial tot =
      reduce_partials(&hdr(0).p, a.node_n, uint32_t(block / sizeof(LwPartial)), dsum, dcnt, dmin, dmax, dor, drf);
  LwBrkCounts C{};
  uint64_t ent = 0;  // rows that entered the node (unknown if any rank's is)
  uint32_t maxmid = 0;
  for (uint32_t k = 0; k < a.node_n; ++k) {
    const LwNodeHdr& rc = hdr(k);
    if (rc.mid[q] <= kNodeCap) maxmid = max(maxmid, rc.mid[q]);  // more misses at any cap
    for (int j = 0; j < kBrkQ; ++j) {
      C.lt[j] += rc.lt[j];
      C.mid[j] += rc.mid[j];
      C.elo[j] += rc.elo[j];
      C.ehi[j] += rc.ehi[j];
    }
    C.ovf |= rc.ovf;
    ent = (ent == ~uint64_t(0) || rc.ent == 0xFFFFFFFFu) ? ~uint64_t(0) : ent + rc.ent;
  }
  // the next refresh's record cap (lw_brk_finish hands the node's most to the host)
  if (t == 0) atomicMax(a.brk_cnt + 1, maxmid);
  lw_brk_resolve(a, s, q, b, tot, C, ent, r, col, keys, hist, tmp, found, red, [&](uint32_t* dst) {
    // the union of the ranks' kept keys of bracket q, rank order
    uint32_t base = 0;
    for (uint32_t k = 0; k < a.node_n; ++k) {
      const uint32_t m = hdr(k).mid[q];
      const uint32_t* src = reinterpret_cast<const uint32_t*>(a.nball + k * block +
                                                              size_t(a.num_series) * sizeof(LwNodeHdr)) +
                            (size_t(s) * kBrkQ + q) * a.node_cap;
      for (uint32_t j = t; j < m; j += NT) dst[base + j] = src[j];
      base += m;
    }
  });
}

// The end of scan B (local and node): every workgroup counts itself done; the last one
// (its device atomic returns the grid size - 1) counts the series the radix chain still has
// to resolve and writes the report word - the host's wait ends one kernel earlier than with
// a separate report launch. Every writer fences before the barrier, the counter's
// increment is a vector atomic on device memory, and the last workgroup resets it.
__device__ inline void lw_brk_finish(const LwArgs& a) {
  __shared__ uint32_t last, left;
  const int t = threadIdx.x;
  __threadfence();
  __syncthreads();
  if (t == 0) {
    left = 0;
    last = atomicAdd(a.brk_cnt, 1u) == gridDim.x * gridDim.y - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  for (uint32_t s = t; s < a.num_series; s += NT)
    if (!a.sel[s].done) atomicAdd(&left, 1u);
  __syncthreads();
  if (t == 0) {
    a.brk_cnt[0] = 0u;
    const uint32_t maxmid = atomicExch(a.brk_cnt + 1, 0u);
    if (a.report)  // one word: no system fence between two stores the host must see in order
      __hip_atomic_store(a.report,
                         (static_cast<unsigned long long>(min(maxmid, 0xFFFFu)) << 48) |
                             (static_cast<unsigned long long>(left) << 24) | (a.params->seq & 0xFFFFFFu),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(NT) void lw_scan_brk(const LwArgs a) {
  lw_scan_brk_body<false>(a);
  lw_brk_finish(a);
}

// scan B with pass B fused in (LongWindowSet::refresh_incremental: a short work list)
__global__ __launch_bounds__(NT) void lw_scan_brk_fused(const LwArgs a) {
  lw_scan_brk_body<true>(a);
  lw_brk_finish(a);
}

__global__ __launch_bounds__(NT) void lw_node_brk_select(const LwArgs a) {
  lw_node_brk_select_body(a);
  lw_brk_finish(a);
}

// A small refresh's staging in one launch: block 0 copies the parameter block and the work
// list from the pinned host slot, blocks 1.. the new rows of one ring segment each from the
// pinned host ring into the device window (rows that cross neither ring's wrap). Replaces
// 2-4 DMA copies whose fixed cost dominated a refresh that changes a few chunks.
// Host reads cross the fabric (microseconds each): a thread issues kIngestBatch of them
// before it stores any, so a copy of a few KB is one round trip, not one per 256 words.
constexpr uint32_t kIngestBatch = 8;
__device__ inline void lw_copy_batched(uint32_t* dst, const uint32_t* src, uint32_t n) {
  for (uint32_t base = threadIdx.x; base < n; base += NT * kIngestBatch) {
    uint32_t v[kIngestBatch];
#pragma unroll
    for (uint32_t k = 0; k < kIngestBatch; ++k) v[k] = base + k * NT < n ? src[base + k * NT] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < kIngestBatch; ++k)
      if (base + k * NT < n) dst[base + k * NT] = v[k];
  }
}
__global__ __launch_bounds__(NT) void lw_ingest(const LwIngest in) {
  if (blockIdx.x == 0) {
    lw_copy_batched(reinterpret_cast<uint32_t*>(in.dp), reinterpret_cast<const uint32_t*>(in.hp),
                    uint32_t(sizeof(LwParams) / 4));
    lw_copy_batched(in.dwork, in.hwork, in.nwork);
    return;
  }
  if (blockIdx.x == 1 + in.nseg) {
    lw_copy_batched(in.bdst, in.bsrc, in.bwords);
    return;
  }
  const LwIngestSeg g = in.seg[blockIdx.x - 1];
  lw_copy_batched(reinterpret_cast<uint32_t*>(g.dst), reinterpret_cast<const uint32_t*>(g.src), g.floats);
}

}  // namespace

void lw_launch_pass_brk(uint32_t grid, hipStream_t stream, const LwArgs& a) {
  hipLaunchKernelGGL(lw_pass_brk, dim3(grid), dim3(NT), 0, stream, a);
}

void lw_launch_scan_brk(bool fused, hipStream_t stream, const LwArgs& a) {
  const dim3 grid(a.num_series, kBrkQ);
  if (fused) hipLaunchKernelGGL(lw_scan_brk_fused, grid, dim3(NT), 0, stream, a);
  else hipLaunchKernelGGL(lw_scan_brk, grid, dim3(NT), 0, stream, a);
}

void lw_launch_node_brk_local(hipStream_t stream, const LwArgs& a) {
  hipLaunchKernelGGL(lw_node_brk_local, dim3(a.num_series), dim3(NT), 0, stream, a);
}

void lw_launch_node_brk_select(hipStream_t stream, const LwArgs& a) {
  hipLaunchKernelGGL(lw_node_brk_select, dim3(a.num_series, kBrkQ), dim3(NT), 0, stream, a);
}

// grid: the parameter block and work list, one workgroup per row segment, the brackets' copy
void lw_launch_ingest(hipStream_t stream, const LwIngest& in) {
  hipLaunchKernelGGL(lw_ingest, dim3(1 + in.nseg + (in.bwords ? 1 : 0)), dim3(NT), 0, stream, in);
}

}  // namespace rocmdash
