// Long-window statistics (see long_window.h): the host class. It plans the chunks, stages
// the new rows and the parameter block, and drives the refreshes - direct launches by
// default, optionally a hipGraph that captured them. The kernels live in
// long_window_radix.hip and long_window_brackets.hip and are reached through the launchers
// of long_window_args.h.
#include "long_window.h"
#include "tagged.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "long_window_args.h"
#include "rccl_comm.h"

namespace rocmdash {
namespace {

constexpr auto check = lw_check;

struct Guard {
  int prev = -1;
  explicit Guard(int dev) {
    (void)hipGetDevice(&prev);
    if (prev != dev) check(hipSetDevice(dev), "hipSetDevice");
  }
  ~Guard() {
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
  }
};

uint64_t ns_since(std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t1) {
  return uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count());
}

}  // namespace

LongWindowSet::LongWindowSet(uint32_t window, int device, bool use_graph, uint32_t chunk_rows)
    : window_(window), device_(device), use_graph_(use_graph), chunk_rows_(chunk_rows) {
  if (const char* e = std::getenv("ROCMDASH_LW_PLAN_ROUNDS")) plan_rounds_ = uint32_t(std::clamp(std::atoi(e), 1, 16));
  if (const char* e = std::getenv("ROCMDASH_LW_BRK_TARGET"))
    brk_target_ = uint32_t(std::clamp(std::atoi(e), 256, int(kBrkTarget)));
  if (chunk_rows && (chunk_rows < 256 || chunk_rows > kLongChunkRows || (chunk_rows & (chunk_rows - 1))))
    throw std::invalid_argument("chunk_rows must be 0 (auto) or a power of two in [256, 32768]");
  if (window < kLongMinWindow || window > kLongMaxWindow || (window & (window - 1)))
    throw std::invalid_argument("long window must be a power of two in [2^10, 2^26]");
  const auto off = [](const char* v) { return v[0] == '0' || v[0] == 'n' || v[0] == 'f'; };
  if (const char* v = std::getenv("ROCMDASH_LW_WAVE_PRIVATE")) wave_priv_ = off(v) ? 0 : (v[0] == '2' ? 2 : 1);
  if (const char* v = std::getenv("ROCMDASH_LW_COMPACT")) compact_ = !off(v);
  if (const char* v = std::getenv("ROCMDASH_LW_PREFETCH")) prefetch_ = std::max(0, std::min(2, std::atoi(v)));
  if (const char* v = std::getenv("ROCMDASH_LW_BRACKETS")) brackets_ = !off(v);
  if (const char* v = std::getenv("ROCMDASH_LW_INCREMENTAL")) incremental_ = !off(v);
}

LongWindowSet::~LongWindowSet() {
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(device_);
  // refreshes still in flight write the work buffers and the host-mapped flags: wait for
  // this set's own last refresh only - never hipDeviceSynchronize, which
  // would also wait for an RCCL kernel stuck on a dead peer and hang the exit. The
  // members then release what they own (last_done_ first, long_window.h)
  if (last_done_) (void)hipEventSynchronize(last_done_.get());
  (void)hipSetDevice(cur);
}

uint32_t LongWindowSet::add_ring(std::shared_ptr<SeriesRing> ring) {
  if (!ring) throw std::invalid_argument("null ring");
  if (part_) throw std::logic_error("add_ring after the first refresh");
  if (rings_.size() == size_t(kLongMaxRings)) throw std::invalid_argument("at most 4 rings per long window set");
  const uint32_t width = ring->width();
  if (width == 0 || width > uint32_t(kLongMaxWidth)) throw std::invalid_argument("ring width must be in [1, 16]");
  Guard g(device_);
  RingState rs;
  rs.ring = std::move(ring);
  rs.first_series = nseries_;
  rs.dev = LwDeviceBuf(size_t(window_) * width * sizeof(float), 0xFF, "hipMalloc long window");  // NaN until written
  if (rs.ring->pinned()) {  // lw_ingest reads the new rows straight from the pinned host ring
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<float*>(rs.ring->rows()), 0) == hipSuccess && d)
      rs.host_dev = static_cast<const float*>(d);
    else
      (void)hipGetLastError();
  }
  nseries_ += width;
  rings_.push_back(std::move(rs));
  return rings_.back().first_series;
}

void LongWindowSet::allocate_work() {
  if (rings_.empty()) throw std::logic_error("no rings");
  plan_chunks();
  const size_t S = nseries_;
  params_ = LwDeviceBuf(sizeof(LwParams));
  LwDeviceBuf part(S * max_chunks_ * sizeof(LwPartial));
  {  // a ring with fewer chunks never writes the slots past them: identity partials
    const std::vector<LwPartial> ident(S * max_chunks_, LwPartial{0.0, 0, 0xFFFFFFFFu, 0, 0, 0, 0});
    check(hipMemcpy(part.get(), ident.data(), ident.size() * sizeof(LwPartial), hipMemcpyHostToDevice), "hipMemcpy");
  }
  hist0_ = LwDeviceBuf(S * kB0 * sizeof(uint32_t), 0);
  histk_ = LwDeviceBuf(S * kLongRanks * 256 * sizeof(uint32_t), 0);
  sel_ = LwDeviceBuf(S * sizeof(LwSel), 0);
  dig0_ = LwDeviceBuf(S * 3 * sizeof(uint32_t));
  constexpr unsigned kStaging = hipHostMallocMapped | hipHostMallocCoherent;
  host_params_ = LwHostBuf(kSlots * sizeof(LwParams), kStaging, false, false);
  slot_done_.clear();
  for (int i = 0; i < kSlots; ++i) slot_done_.push_back(lw_make_event(hipEventDisableTiming));
  {
    hipStream_t s = nullptr;
    check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
    cap_stream_ = LwStream(s);
  }
  last_done_ = lw_make_event(hipEventDisableTiming);
  // the incremental pass B's work lists: one pinned staging list per parameter slot
  work_dev_ = LwDeviceBuf(size_t(pass_wgs_) * sizeof(uint32_t));
  work_host_ = LwHostBuf(size_t(kSlots) * pass_wgs_ * sizeof(uint32_t), kStaging, false, false);
  allocate_mode(0);  // the local refresh's brackets (the node's at its first refresh_node)
  part_ = std::move(part);  // last: part_ marks the work buffers as allocated
}

// One bracket state (0: local refreshes, 1: node refreshes - around different percentiles,
// so neither invalidates the other's chunk counts): the brackets, pass B's per-chunk
// counts and kept-key slabs (3 / 64 of the window per series, lw_qcap), and the host-mapped
// flags the kernels leave for the host (wants brackets, brackets changed, the report word).
void LongWindowSet::allocate_mode(int mode) {
  if (bm_[mode].brk) return;
  const size_t S = nseries_;
  BrkMode m;
  m.brk = LwDeviceBuf(S * sizeof(LwBrk), 0);  // no brackets: the first refresh takes the radix chain
  m.brk_used = LwDeviceBuf(S * sizeof(LwBrk), 0);
  m.bpart = LwDeviceBuf(S * max_chunks_ * sizeof(LwBrkPart), 0);
  m.bcand = LwDeviceBuf(std::max<size_t>(1, bcand_keys_) * sizeof(uint32_t), -1, "hipMalloc slabs");
  m.hflags = LwHostBuf(S * sizeof(uint32_t), hipHostMallocMapped, true, true);
  m.bchg = LwHostBuf(S * sizeof(uint32_t), hipHostMallocMapped, true, true);
  m.report = LwHostBuf(sizeof(unsigned long long), hipHostMallocMapped, true, true);
  m.brk_cnt = LwDeviceBuf(2 * sizeof(uint32_t), 0);
  m.done = lw_make_event(hipEventDisableTiming);
  m.seg_head.assign(2 * kLongMaxRings, kNever);
  bm_[mode] = std::move(m);
}

std::vector<std::pair<uint32_t, uint32_t>> long_window_chunk_plan(uint32_t window, const std::vector<uint32_t>& widths,
                                                                  int cus, uint32_t chunk_rows, uint32_t rounds) {
  // inputs of the exposed free function are checked here: the search below
  // ends for every valid window, and is bounded anyway
  if (window < kLongMinWindow || window > kLongMaxWindow || (window & (window - 1)))
    throw std::invalid_argument("long_window_chunk_plan: window must be a power of two in [2^10, 2^26]");
  if (widths.empty() || widths.size() > size_t(kLongMaxRings))
    throw std::invalid_argument("long_window_chunk_plan: 1 to 4 ring widths");
  for (uint32_t w : widths)
    if (w == 0 || w > uint32_t(kLongMaxWidth)) throw std::invalid_argument("long_window_chunk_plan: widths in [1, 16]");
  if (chunk_rows && (chunk_rows < 256 || chunk_rows > kLongChunkRows || (chunk_rows & (chunk_rows - 1))))
    throw std::invalid_argument("long_window_chunk_plan: chunk_rows must be 0 or a power of two in [256, 32768]");
  if (rounds < 1 || rounds > 16) throw std::invalid_argument("long_window_chunk_plan: rounds in [1, 16]");
  std::vector<std::pair<uint32_t, uint32_t>> plan(widths.size());
  if (chunk_rows) {  // uniform chunks (the caller's; tests and A/B)
    for (auto& p : plan) p = {chunk_rows, std::max<uint32_t>(1, window / chunk_rows)};
    return plan;
  }
  // Balanced by bytes: the passes are latency-bound per wave, so a pass lasts as long as
  // its slowest workgroup. Equal rows per workgroup over an 8-series and a 4-series ring
  // leave the 4-series workgroups done at half time and the chip at half occupancy for
  // the rest (profiles/r04/lw_ab/). Instead every workgroup streams about the same
  // bytes, and the grid is one round of the chip's workgroup slots (4 per CU at the
  // passes' registers) - or whole rounds, when a ring would need more rows per workgroup
  // than its 16-bit LDS bins allow. Rows per workgroup: a multiple of 256, >= 256.
  uint32_t total = 0;
  for (uint32_t w : widths) total += w;
  const uint64_t slots = uint64_t(std::max(cus, 1)) * 4;
  // every ring fits once a segment's workgroups reach window / kLongChunkRowsMax: at most
  // that many rounds of the slots
  const uint64_t max_rounds = uint64_t(kLongMaxWindow) / 256 + 1;
  for (uint64_t G = slots * rounds, round = 0; round < max_rounds; G += slots, ++round) {
    bool fits = true;
    for (size_t i = 0; i < widths.size() && fits; ++i) {
      const uint32_t nseg = (widths[i] + kSegCols - 1) / kSegCols;
      const double share = double(G) * widths[i] / double(std::max(total, 1u)) / nseg;  // workgroups per segment
      const uint64_t wg = std::max<uint64_t>(1, uint64_t(share + 0.5));
      uint64_t rows = (uint64_t(window) + wg - 1) / wg;
      rows = std::max<uint64_t>(256, (rows + 255) / 256 * 256);
      if (rows > kLongChunkRowsMax) fits = false;
      else plan[i] = {uint32_t(rows), uint32_t((uint64_t(window) + rows - 1) / rows)};
    }
    if (fits) {
      if (rounds > 1) {
        // an incremental plan: every ring takes the smallest ring chunk - pass B's
        // column-split workgroups stream chunk_rows rows whatever the ring's width, so the
        // steady refresh waits for the longest chunk, not the widest ring
        uint32_t rmin = plan[0].first;
        for (const auto& p : plan) rmin = std::min(rmin, p.first);
        for (auto& p : plan) p = {rmin, uint32_t((uint64_t(window) + rmin - 1) / rmin)};
      }
      return plan;
    }
  }
  throw std::logic_error("long_window_chunk_plan: no plan found");
}

void LongWindowSet::plan_chunks() {
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_);
  std::vector<uint32_t> widths;
  for (const auto& r : rings_) widths.push_back(r.ring->width());
  const auto plan = long_window_chunk_plan(window_, widths, cus, chunk_rows_, plan_rounds_);
  max_chunks_ = 1;
  cand_cap_ = 1;
  pass_wgs_ = 0;
  bcand_keys_ = 0;
  seg_cols_.clear();
  for (size_t i = 0; i < rings_.size(); ++i) {
    auto& r = rings_[i];
    r.chunk_rows = plan[i].first;
    r.nchunks = plan[i].second;
    r.qcap = lw_qcap(r.chunk_rows);
    r.bstride = uint64_t(r.nchunks) * kBrkQ * r.qcap;
    r.boff = bcand_keys_;
    bcand_keys_ += r.bstride * widths[i];
    max_chunks_ = std::max(max_chunks_, r.nchunks);
    cand_cap_ = std::max(cand_cap_, r.nchunks * r.chunk_rows);
    for (uint32_t c0 = 0; c0 < widths[i]; c0 += kSegCols) {  // the flat pass grid: every segment's chunks
      seg_cols_.push_back(std::min(kSegCols, widths[i] - c0));
      pass_wgs_ += r.nchunks;
    }
  }
}

LwArgs LongWindowSet::make_args(float* out, int mode, bool brk, bool incr) const {
  LwArgs a{};
  for (size_t i = 0; i < rings_.size(); ++i) {
    const auto& r = rings_[i];
    a.rings[i] = LwRing{r.dev.get<float>(), r.ring->width(), r.first_series, r.chunk_rows, r.nchunks, r.qcap, 0u,
                        r.boff,             r.bstride};
  }
  a.num_rings = uint32_t(rings_.size());
  a.num_segs = 0;
  uint32_t wg0 = 0;
  for (uint32_t i = 0; i < a.num_rings; ++i)
    for (uint32_t c0 = 0; c0 < rings_[i].ring->width(); c0 += kSegCols) {
      a.segs[a.num_segs++] = LwSeg{i, c0, std::min(kSegCols, rings_[i].ring->width() - c0), wg0};
      wg0 += rings_[i].nchunks;
    }
  a.num_series = nseries_;
  a.mask = window_ - 1;
  a.max_chunks = max_chunks_;
  a.params = params_.get<LwParams>();
  a.part = part_.get<LwPartial>();
  a.hist0 = hist0_.get<uint32_t>();
  a.histk = histk_.get<uint32_t>();
  a.sel = sel_.get<LwSel>();
  a.dig0 = dig0_.get<uint32_t>();
  a.out = out;
  a.wave_priv = uint32_t(wave_priv_);
  const BrkMode& m = bm_[mode];
  a.brk_on = brk ? 1u : 0u;
  a.brk = m.brk.get<LwBrk>();
  a.brk_used = m.brk_used.get<LwBrk>();
  a.hflags = m.hflags.dev<uint32_t>();
  a.bpart = m.bpart.get<LwBrkPart>();
  a.bcand = m.bcand.get<uint32_t>();
  a.incr = incr ? 1u : 0u;
  a.work = work_dev_.get<uint32_t>();
  a.nwork = 0;
  a.bchg = m.bchg.dev<uint32_t>();
  a.report = m.report.dev<unsigned long long>();
  a.brk_cnt = m.brk_cnt.get<uint32_t>();
  a.brk_target = brk_target_;
  a.dbg = dbg_.get<unsigned long long>();
  // candidate compaction (pass 2 -> pass 3), its own slabs
  a.compact = compact_ ? 1u : 0u;
  a.cand = compact_ ? cand_.get<uint32_t>() : nullptr;
  a.cand_n = compact_ ? cand_n_.get<uint32_t>() : nullptr;
  a.cand_cap = cand_cap_;
  return a;
}

size_t LongWindowSet::lds_bytes(int pass) const {
  uint32_t maxw = 0;  // series per segment
  for (const auto& r : rings_) maxw = std::max(maxw, std::min(kSegCols, r.ring->width()));
  if (pass == 0)  // one 10-bit copy, 4 per-wave 8-bit copies, or 8 per-half-wave ones (+16 words each)
    return std::max<size_t>(size_t(maxw) * (kB0 / 2), wave_priv_ == 2 ? 8 * (size_t(maxw) * 128 + 16) : 0) *
           sizeof(uint32_t);
  return size_t(maxw) * kLongRanks * 128 * sizeof(uint32_t);
}

void LongWindowSet::check_args(const LwArgs& a) const {
  // the slabs pass B and pass 2 write must exist before any kernel indexes them
  if (a.compact && (a.cand == nullptr || a.cand_n == nullptr || cand_cap_ < window_))
    throw std::logic_error("long window: compaction buffers missing");
  if (a.brk_on && (a.bcand == nullptr || a.bpart == nullptr || a.brk == nullptr || a.brk_used == nullptr))
    throw std::logic_error("long window: bracket buffers missing");
}

// The radix chain (passes 0-3 with their scans); series scan B resolved are skipped. The
// node refresh hooks its two extra kernels and its collectives in between.
void LongWindowSet::enqueue_chain(hipStream_t stream, const LwArgs& a, const ChainHooks& hooks) {
  if (hooks.before_pass0) hooks.before_pass0();
  for (int k = 0; k < 4; ++k) {
    if (k == 3 && a.compact) lw_launch_pass_cand(stream, a);
    else lw_launch_pass(k, prefetch_, pass_wgs_, lds_bytes(k), stream, a);
    if (k == 0 && hooks.after_pass0) hooks.after_pass0();
    if (k > 0 && hooks.after_pass) hooks.after_pass(k);
    lw_launch_scan(k, stream, a);
  }
  st_.kernel_launches += 8;
}

void LongWindowSet::enqueue_passes(hipStream_t stream, float* out, bool brk) {
  const LwArgs a = make_args(out, 0, brk, false);
  check_args(a);
  if (a.brk_on) {  // bracket mode: pass B + scan B, then the radix chain for what they left
    lw_launch_pass_brk(pass_wgs_, stream, a);
    lw_launch_scan_brk(false, stream, a);
    st_.kernel_launches += 2;
  }
  enqueue_chain(stream, a);
  check(hipGetLastError(), "long-window launch");
}

void LongWindowSet::stage(hipStream_t stream, float p0, float p1, float p2) {
  if (!part_) allocate_work();
  if (compact_ && !cand_) {  // pass 2's candidate slabs: one key per window sample at most
    const size_t chunks = max_chunks_;
    cand_ = LwDeviceBuf(size_t(nseries_) * cand_cap_ * sizeof(uint32_t), -1, "hipMalloc cand");
    cand_n_ = LwDeviceBuf(size_t(nseries_) * chunks * sizeof(uint32_t), -1, "hipMalloc cand_n");
    check(hipMemsetAsync(cand_n_.get(), 0, cand_n_.bytes(), stream), "hipMemsetAsync");
  }
  const uint64_t W = window_;
  LwParams P{};
  // a small refresh - every ring pinned (device-visible), no lost rows, few rows in all -
  // stages through lw_ingest (flush_stage) instead of DMA copies
  ingest_segs_.clear();
  ingest_pending_ = host_params_.dev() != nullptr && work_host_.dev() != nullptr;
  {
    uint64_t floats = 0;
    for (const auto& r : rings_) {
      const uint64_t h = r.ring->head();
      const uint64_t lo = std::max<uint64_t>(r.copied, h > W ? h - W : 0);
      if (!r.host_dev || h - lo > r.ring->capacity()) ingest_pending_ = false;
      floats += (h - lo) * r.ring->width();
    }
    if (floats * sizeof(float) > kIngestMaxBytes) ingest_pending_ = false;
  }
  for (size_t i = 0; i < rings_.size(); ++i) {
    auto& r = rings_[i];
    const SeriesRing& ring = *r.ring;
    const uint32_t width = ring.width();
    const uint64_t cap = ring.capacity();
    const uint64_t h = ring.head();
    uint64_t lo = std::max<uint64_t>(r.copied, h > W ? h - W : 0);  // older rows leave the window anyway
    if (h - lo > cap) {
      // the host ring overwrote rows [lo, h - cap) before this refresh: NaN in the window
      const uint64_t lost_end = h - cap;
      st_.rows_lost += lost_end - lo;
      while (lo < lost_end) {
        const uint64_t seg_end = std::min<uint64_t>(lost_end, (lo / W + 1) * W);
        check(hipMemsetAsync(r.dev.get<float>() + (lo & (W - 1)) * width, 0xFF, size_t(seg_end - lo) * width * sizeof(float), stream),
              "hipMemsetAsync");
        lo = seg_end;
      }
    }
    // copy [lo, h) in segments that cross neither the device wrap (multiple of W) nor
    // the host wrap (multiple of cap): both powers of two, so split at the smaller
    const uint64_t m = std::min<uint64_t>(W, cap);
    while (lo < h) {
      const uint64_t seg_end = std::min<uint64_t>(h, (lo / m + 1) * m);
      const size_t bytes = size_t(seg_end - lo) * width * sizeof(float);
      if (ingest_pending_) {
        ingest_segs_.push_back({uint64_t(i), lo, seg_end - lo});
      } else {
        check(hipMemcpyAsync(r.dev.get<float>() + (lo & (W - 1)) * width, ring.rows() + (lo & (cap - 1)) * width, bytes,
                             hipMemcpyHostToDevice, stream),
              "hipMemcpyAsync");
        ++st_.memcpy_calls;
      }
      st_.rows_copied += seg_end - lo;
      st_.bytes_copied += bytes;
      lo = seg_end;
    }
    r.copied = h;
    P.head[i] = h;
    P.prev_head[i] = r.last_head;  // pass 0 predicts the varying key bits from what entered since
    r.last_head = h;
    P.n[i] = uint32_t(std::min<uint64_t>(h, W));
  }
  P.pct[0] = p0;
  P.pct[1] = p1;
  P.pct[2] = p2;
  P.seq = ++seq_;
  // parameter block: pinned staging slot (reused only once its copy has executed)
  const uint32_t slot = slot_++ % kSlots;
  cur_slot_ = slot;
  check(hipEventSynchronize(slot_done_[slot].get()), "hipEventSynchronize");
  LwParams* hp = host_params_.host<LwParams>() + slot;
  std::memcpy(hp, &P, sizeof P);
  if (ingest_pending_) return;  // lw_ingest copies the block (flush_stage)
  check(hipMemcpyAsync(params_.get(), hp, sizeof P, hipMemcpyHostToDevice, stream), "hipMemcpyAsync params");
  // (the slot's event is recorded by the caller, after the work list that shares it)
}

void LongWindowSet::flush_stage(hipStream_t stream, uint32_t nwork, int copy_brk_mode) {
  if (!ingest_pending_) return;
  ingest_pending_ = false;
  LwIngest in{};
  in.hp = host_params_.dev<const LwParams>() + cur_slot_;
  in.dp = params_.get<LwParams>();
  in.hwork = work_host_.dev<const uint32_t>() + size_t(cur_slot_) * pass_wgs_;
  in.dwork = work_dev_.get<uint32_t>();
  in.nwork = nwork;
  for (const auto& sg : ingest_segs_) {
    const auto& r = rings_[sg[0]];
    const uint32_t width = r.ring->width();
    const uint64_t cap = r.ring->capacity();
    LwIngestSeg& g = in.seg[in.nseg++];
    g.src = r.host_dev + (sg[1] & (cap - 1)) * width;
    g.dst = r.dev.get<float>() + (sg[1] & (uint64_t(window_) - 1)) * width;
    g.floats = uint32_t(sg[2] * width);
  }
  if (copy_brk_mode >= 0) {  // the fused pass B's brackets (its first workgroup cannot copy them)
    in.bsrc = bm_[copy_brk_mode].brk.get<const uint32_t>();
    in.bdst = bm_[copy_brk_mode].brk_used.get<uint32_t>();
    in.bwords = uint32_t(nseries_ * sizeof(LwBrk) / sizeof(uint32_t));
  }
  lw_launch_ingest(stream, in);
  check(hipGetLastError(), "long-window ingest launch");
  ++st_.ingest_launches;
}

// a refresh with no bracket step: the staging (no work list) and the parameter slot's event
void LongWindowSet::finish_stage(hipStream_t stream) {
  flush_stage(stream, 0);
  check(hipEventRecord(slot_done_[cur_slot_].get(), stream), "hipEventRecord");
}

// Incremental pass B's work list (long_window.h). Needs the previous refresh of the bracket
// state complete (its flags final): the caller synchronised on it.
std::vector<uint32_t> long_window_work_list(uint32_t window, const LwWorkRing* rings, size_t nrings,
                                            uint64_t* seg_head, const uint32_t* want_flags,
                                            const uint32_t* changed) {
  std::vector<uint32_t> work;
  const uint64_t W = window;
  uint32_t g = 0, s0 = 0;
  for (size_t i = 0; i < nrings; ++i) {
    const LwWorkRing& r = rings[i];
    const uint64_t h = r.copied;
    for (uint32_t c0 = 0; c0 < r.width; c0 += kSegCols, ++g) {
      const uint32_t ncols = std::min(kSegCols, r.width - c0);
      bool want = false, full = seg_head[g] == kLongNever || h < seg_head[g] || h - seg_head[g] >= W;
      for (uint32_t col = 0; col < ncols; ++col) {
        const uint32_t s = s0 + c0 + col;
        want = want || want_flags[s] != 0;
        full = full || changed[s] != 0;
      }
      if (!want) {  // pass B does not look at this segment: its counts go stale
        seg_head[g] = kLongNever;
        continue;
      }
      if (full) {
        for (uint32_t c = 0; c < r.nchunks; ++c) work.push_back((g << 20) | c);
      } else if (h > seg_head[g]) {
        // slots [lo, hi) of the device ring, possibly wrapping
        const uint64_t lo = seg_head[g] & (W - 1), n = h - seg_head[g];
        const uint32_t c_lo = uint32_t(lo / r.chunk_rows), c_hi = uint32_t(((lo + n - 1) & (W - 1)) / r.chunk_rows);
        if (lo + n <= W) {
          for (uint32_t c = c_lo; c <= c_hi; ++c) work.push_back((g << 20) | c);
        } else {
          for (uint32_t c = c_lo; c < r.nchunks; ++c) work.push_back((g << 20) | c);
          for (uint32_t c = 0; c <= c_hi && c < c_lo; ++c) work.push_back((g << 20) | c);
        }
      }
      seg_head[g] = h;
    }
    s0 += r.width;
  }
  return work;
}

// Pass B's grid from the work list (long_window.h): a short list is split by column (one
// workgroup per (chunk, series): the same counts and sums, spread over more CUs). Nothing
// changed at all: one workgroup still runs - the grid's first copies the brackets scan B
// decides with (lw_pass_body) - on a chunk whose counts it rewrites unchanged.
LwWorkShape long_window_shape_work(std::vector<uint32_t> work, const std::vector<uint32_t>& seg_cols,
                                   uint32_t flat_grid, uint32_t fuse_chunks, size_t split_max, bool fuse) {
  LwWorkShape sh;
  if (!work.empty() && work.size() >= flat_grid) {  // every chunk: the flat grid, no list
    sh.grid = flat_grid;
    return sh;
  }
  // fused pass B: the segments with at most fuse_chunks changed chunks are streamed by scan
  // B's own workgroups (lw_scan_brk_fused); a segment with more (its brackets moved: every
  // chunk) keeps pass B
  if (fuse) {
    std::vector<uint32_t> per(seg_cols.size(), 0);
    for (uint32_t e : work) ++per[e >> 20];
    std::vector<uint32_t> rest;
    for (uint32_t e : work) (per[e >> 20] <= fuse_chunks ? sh.fused : rest).push_back(e);
    work.swap(rest);
  }
  if (work.empty() && !fuse) work.push_back(0u);  // pass B's first workgroup copies brk -> brk_used
  if (!work.empty()) {
    size_t split_n = 0;
    for (uint32_t e : work) split_n += seg_cols[e >> 20];
    if (split_n + sh.fused.size() <= flat_grid && split_n <= split_max) {
      std::vector<uint32_t> sw;
      sw.reserve(split_n);
      for (uint32_t e : work)
        for (uint32_t col = 0; col < seg_cols[e >> 20]; ++col)
          sw.push_back(((e >> 20) << 23) | (col << 20) | (e & 0xFFFFFu));
      work.swap(sw);
      sh.colsplit = true;
    }
  }
  sh.grid = uint32_t(work.size());
  sh.pass = std::move(work);
  return sh;
}

// Incremental pass B's grid for bracket state `mode`: the work list, shaped, uploaded
// through the parameter slot's pinned staging (pass B's entries, then the fused ones) with
// whatever staging is still pending. fuse: allowed; it also needs lw_ingest's staging.
uint32_t LongWindowSet::upload_work(hipStream_t stream, LwArgs& a, int mode, uint32_t slot, bool fuse,
                                    bool* fused) {
  BrkMode& m = bm_[mode];
  LwWorkRing rings[kLongMaxRings];
  for (size_t i = 0; i < rings_.size(); ++i)
    rings[i] = LwWorkRing{rings_[i].ring->width(), rings_[i].chunk_rows, rings_[i].nchunks, rings_[i].copied};
  uint32_t* bchg = m.bchg.host<uint32_t>();
  std::vector<uint32_t> list =
      long_window_work_list(window_, rings, rings_.size(), m.seg_head.data(), m.hflags.host<uint32_t>(), bchg);
  for (uint32_t s = 0; s < nseries_; ++s) bchg[s] = 0;  // consumed (the kernels set them again)
  st_.passb_chunks += list.size();
  *fused = fuse && ingest_pending_;
  const LwWorkShape sh = long_window_shape_work(std::move(list), seg_cols_, pass_wgs_, kFuseChunks, kSplitMax, *fused);
  a.colsplit = sh.colsplit ? 1u : 0u;
  a.nfused = 0;
  if (sh.grid == pass_wgs_ && sh.pass.empty()) {  // every chunk: the flat grid
    *fused = false;
    flush_stage(stream, 0);
    return pass_wgs_;
  }
  const size_t nall = sh.pass.size() + sh.fused.size();  // <= pass_wgs_ (the slot's and the device list's size)
  uint32_t* wh = work_host_.host<uint32_t>() + size_t(slot) * pass_wgs_;
  if (!sh.pass.empty()) std::memcpy(wh, sh.pass.data(), sh.pass.size() * sizeof(uint32_t));
  if (!sh.fused.empty()) std::memcpy(wh + sh.pass.size(), sh.fused.data(), sh.fused.size() * sizeof(uint32_t));
  a.nwork = uint32_t(sh.pass.size());
  a.fwork = work_dev_.get<uint32_t>() + sh.pass.size();
  a.nfused = uint32_t(sh.fused.size());
  if (*fused) {
    flush_stage(stream, uint32_t(nall), mode);  // rows, parameters, both lists and brk -> brk_used
    ++st_.fused_refreshes;
    std::vector<bool> seen(a.num_segs, false);
    for (uint32_t e : sh.fused)
      if (!seen[e >> 20]) {
        seen[e >> 20] = true;
        ++st_.fused_segments;
      }
  } else if (ingest_pending_) {
    flush_stage(stream, a.nwork);  // rows, parameters and this list in one kernel
  } else {
    check(hipMemcpyAsync(work_dev_.get(), wh, sh.pass.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream),
          "hipMemcpyAsync work");
  }
  return a.nwork;
}

// Wait for the report word of refresh `seq` (lw_brk_finish); returns the series the radix
// chain still has to resolve. Bounded: a device that never gets there is an error.
uint32_t LongWindowSet::wait_report(int mode, uint32_t seq, double timeout_s, uint32_t* maxmid,
                                   const std::function<bool()>* abandon) {
  volatile unsigned long long* w = bm_[mode].report.host<volatile unsigned long long>();
  const auto t0 = std::chrono::steady_clock::now();
  const auto t_end = t0 + std::chrono::duration<double>(timeout_s);
  auto t_poll = t0 + std::chrono::milliseconds(20);
  SpinBackoff wait;  // tagged.h: spin, then sleep-poll (node mode waits for its peers here)
  for (;;) {
    const unsigned long long v = *w;
    if (uint32_t(v & 0xFFFFFFu) == (seq & 0xFFFFFFu)) {  // seq mod 2^24: the previous refresh's differs
      if (maxmid) *maxmid = uint32_t(v >> 48);
      return uint32_t(v >> 24) & 0xFFFFFFu;
    }
    if (wait.pause()) {
      const auto now = std::chrono::steady_clock::now();
      if (now > t_end)
        throw std::runtime_error("long window: the bracket report of refresh " + std::to_string(seq) +
                                 " never arrived (device hung or a collective waits for a lost rank)");
      if (abandon && *abandon && now >= t_poll) {
        t_poll = now + std::chrono::milliseconds(20);
        if ((*abandon)())
          throw std::runtime_error("long window: node refresh " + std::to_string(seq) +
                                   " abandoned (the node moved on to a newer epoch)");
      }
    }
  }
}

// The bracket step of a refresh (local and node): pass B over the work list, the mode's
// scan B, the report; the host waits for it and the caller launches the radix chain only
// when some series needs it.
uint32_t LongWindowSet::bracket_step(hipStream_t stream, LwArgs& a, const BracketStep& step,
                                     const std::function<void(bool)>& resolve) {
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  ++st_.bracket_refreshes;
  const uint32_t slot = cur_slot_;
  bool fused = false;
  const uint32_t grid = upload_work(stream, a, step.mode, slot, step.fuse, &fused);
  if (grid) {  // pass B for the segments it streams (all of them unless fused)
    lw_launch_pass_brk(grid, stream, a);
    ++st_.kernel_launches;
  }
  if (fused && !grid) ++st_.single_kernel_refreshes;
  resolve(fused);
  check(hipEventRecord(slot_done_[slot].get(), stream), "hipEventRecord");
  check(hipGetLastError(), step.mode == 0 ? "long-window launch" : "long-window node launch");
  const auto t1 = clk::now();
  const uint32_t left = wait_report(step.mode, seq_, step.timeout_s, step.maxmid, step.abandon);
  if (step.host_times) {
    st_.host_enqueue_ns += ns_since(t0, t1);
    st_.host_wait_ns += ns_since(t1, clk::now());
  }
  return left;
}

// Incremental bracket refresh (local): the bracket step, then the radix chain only when
// some series needs it.
void LongWindowSet::refresh_incremental(hipStream_t stream, float* out) {
  BrkMode& m = bm_[0];
  check(hipEventSynchronize(m.done.get()), "hipEventSynchronize");  // the previous refresh's flags are final
  bool brk = false;
  for (uint32_t i = 0; i < nseries_ && !brk; ++i) brk = m.hflags.host<uint32_t>()[i] != 0;
  LwArgs a = make_args(out, 0, brk, true);
  check_args(a);
  uint32_t left = nseries_;
  if (brk) {
    left = bracket_step(stream, a, BracketStep{0, fuse_, true, 60.0, nullptr, nullptr}, [&](bool fused) {
      lw_launch_scan_brk(fused, stream, a);  // fused: scan B streams the short segments' chunks itself
      ++st_.kernel_launches;
    });
  } else {
    finish_stage(stream);
  }
  if (left) {
    ++st_.chain_refreshes;
    enqueue_chain(stream, a);
    check(hipGetLastError(), "long-window launch");
  }
  check(hipEventRecord(m.done.get(), stream), "hipEventRecord");
}

void LongWindowSet::refresh(float* out, void* stream_ptr, float p0, float p1, float p2) {
  auto stream = static_cast<hipStream_t>(stream_ptr);
  Guard g(device_);
  const auto t0 = std::chrono::steady_clock::now();
  stage(stream, p0, p1, p2);
  st_.host_stage_ns += ns_since(t0, std::chrono::steady_clock::now());
  if (brackets_ && incremental_ && !use_graph_) {
    refresh_incremental(stream, out);
  } else {
    finish_stage(stream);
    // bracket mode this refresh: pass B + scan B only when some series wants brackets (the
    // kernels' hint in host memory, from an earlier refresh: a stale hint costs time,
    // never exactness - the radix chain resolves whatever scan B does not). A graph keeps
    // the launches it captured.
    bool any = false;
    for (uint32_t i = 0; i < nseries_ && !any; ++i) any = bm_[0].hflags.host<volatile uint32_t>()[i] != 0;
    const bool brk = brackets_ && (use_graph_ || any);
    if (brk) ++st_.bracket_refreshes;
    if (use_graph_) {
      if (!exec_ || graph_out_ != out || exec_stale_) {
        exec_stale_ = false;
        exec_.reset();
        graph_.reset();
        check(hipStreamBeginCapture(cap_stream_.get(), hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
        const uint64_t launches = st_.kernel_launches;
        enqueue_passes(cap_stream_.get(), out, brk);
        st_.kernel_launches = launches;  // replayed as one graph launch
        hipGraph_t graph = nullptr;
        check(hipStreamEndCapture(cap_stream_.get(), &graph), "hipStreamEndCapture");
        graph_ = LwGraph(graph);
        hipGraphExec_t exec = nullptr;
        check(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0), "hipGraphInstantiate");
        exec_ = LwGraphExec(exec);
        graph_out_ = out;
      }
      check(hipGraphLaunch(exec_.get(), stream), "hipGraphLaunch");
      ++st_.graph_launches;
    } else {
      enqueue_passes(stream, out, brk);
    }
    // every series' chunk counts are stale for the incremental mode after this
    for (auto& h : bm_[0].seg_head) h = kNever;
  }
  check(hipEventRecord(last_done_.get(), stream), "hipEventRecord");
  ++st_.refreshes;
}

uint32_t long_window_node_cap(uint32_t maxmid, uint32_t nranks) { return lw_node_cap_next(maxmid, nranks); }

void LongWindowSet::allocate_node(int nranks) {
  const size_t S = nseries_;
  if (node_ranks_ == nranks) return;
  pred_local_ = LwDeviceBuf(S * sizeof(LwPred));
  pred_all_ = LwDeviceBuf(size_t(nranks) * S * sizeof(LwPred));
  agg_local_ = LwDeviceBuf(S * sizeof(LwPartial));
  agg_all_ = LwDeviceBuf(size_t(nranks) * S * sizeof(LwPartial));
  nbl_ = LwDeviceBuf(lw_node_block(uint32_t(S), kNodeCap));
  nball_ = LwDeviceBuf(size_t(nranks) * lw_node_block(uint32_t(S), kNodeCap));
  node_cap_ = kNodeCap;  // until a bracket refresh has measured the node's kept keys
  if (node_events_.empty())
    for (int i = 0; i < 2 * kNodeCollectives; ++i) node_events_.push_back(lw_make_event(hipEventDefault));
  node_ranks_ = nranks;
}

void LongWindowSet::reset_node() {
  Guard g(device_);
  if (last_done_) check(hipEventSynchronize(last_done_.get()), "hipEventSynchronize");
  BrkMode& m = bm_[1];
  if (m.brk) {
    check(hipEventSynchronize(m.done.get()), "hipEventSynchronize");
    const size_t S = nseries_;
    m.brk.fill(0);  // no brackets: the radix chain first
    m.brk_used.fill(0);
    m.bpart.fill(0);
    m.brk_cnt.fill(0);
    check(hipDeviceSynchronize(), "hipDeviceSynchronize");  // done before any stream reads them
    std::memset(m.hflags.host(), 0, S * sizeof(uint32_t));
    std::memset(m.bchg.host(), 0, S * sizeof(uint32_t));
    m.seg_head.assign(m.seg_head.size(), kNever);
  }
  node_cap_ = kNodeCap;
  node_maxmid_ = 0;
  ++st_.node_resets;
}

void LongWindowSet::set_node_brackets(uint32_t s, const std::vector<uint32_t>& lo, const std::vector<uint32_t>& hi) {
  if (s >= nseries_ || lo.size() != size_t(kBrkQ) || hi.size() != size_t(kBrkQ))
    throw std::invalid_argument("set_node_brackets: a series index and 3 lo / 3 hi keys");
  for (int q = 0; q < kBrkQ; ++q)
    if (lo[q] > hi[q]) throw std::invalid_argument("set_node_brackets: lo > hi");
  Guard g(device_);
  allocate_mode(1);
  if (last_done_) check(hipEventSynchronize(last_done_.get()), "hipEventSynchronize");
  BrkMode& m = bm_[1];
  check(hipEventSynchronize(m.done.get()), "hipEventSynchronize");
  LwBrk b{};
  auto* dev = m.brk.get<LwBrk>() + s;
  check(hipMemcpy(&b, dev, sizeof(LwBrk), hipMemcpyDeviceToHost), "hipMemcpy bracket");
  for (int q = 0; q < kBrkQ; ++q) {
    b.lo[q] = lo[q];
    b.hi[q] = hi[q];
    b.nounion[q] = 0u;
    b.dsave[q] = 0u;
  }
  b.valid = 1u;
  check(hipMemcpy(dev, &b, sizeof(LwBrk), hipMemcpyHostToDevice), "hipMemcpy bracket");
  m.hflags.host<uint32_t>()[s] = 1u;
  m.bchg.host<uint32_t>()[s] = 1u;  // every chunk of the series is counted again
}

void LongWindowSet::refresh_node(float* out, void* stream_ptr, float p0, float p1, float p2, RcclComm* comm,
                                 bool timing, double timeout_s, const std::function<bool()>& abandon) {
  auto stream = static_cast<hipStream_t>(stream_ptr);
  Guard g(device_);
  const int nranks = comm ? comm->nranks() : 1;
  stage(stream, p0, p1, p2);
  allocate_node(nranks);
  allocate_mode(1);  // the node's own brackets: never the local ones
  BrkMode& m = bm_[1];
  // Node bracket mode: the node's brackets are the same on every rank (every kernel that
  // writes them reads only all-gathered data), and so are the flags they leave: once the
  // previous node refresh completed, every rank takes the same branch below - the same
  // collectives in the same order
  const bool use_brk = brackets_ && incremental_ && !use_graph_ && nranks <= int(kNodeBrkRanks);
  bool any = false;
  if (use_brk) {
    check(hipEventSynchronize(m.done.get()), "hipEventSynchronize");
    for (uint32_t i = 0; i < nseries_ && !any; ++i) any = m.hflags.host<uint32_t>()[i] != 0;
  }
  const bool brk = use_brk && any;
  LwArgs a = make_args(out, 1, brk, use_brk);
  a.node_n = uint32_t(nranks);
  a.pred_local = pred_local_.get<LwPred>();
  a.pred_all = (comm ? pred_all_ : pred_local_).get<const LwPred>();
  a.agg_local = agg_local_.get<LwPartial>();
  a.agg_all = (comm ? agg_all_ : agg_local_).get<const LwPartial>();
  a.node_brk = 1;
  a.nbl = nbl_.get<unsigned char>();
  a.nball = (comm ? nball_ : nbl_).get<const unsigned char>();
  a.node_cap = node_cap_;
  check_args(a);
  const size_t S = nseries_;
  timed_ = timing && comm;
  for (auto& f : node_timed_) f = false;
  // the node's collectives on this stream, between the kernels that consume them
  auto collective = [&](int k, auto&& fn) {
    if (!comm) return;
    if (timed_) check(hipEventRecord(node_events_[2 * k].get(), stream), "hipEventRecord");
    fn();
    if (timed_) {
      check(hipEventRecord(node_events_[2 * k + 1].get(), stream), "hipEventRecord");
      node_timed_[k] = true;
    }
  };
  uint32_t left = nseries_;
  if (brk) {
    uint32_t maxmid = 0;
    left = bracket_step(stream, a, BracketStep{1, false, false, timeout_s, &abandon, &maxmid}, [&](bool) {
      lw_launch_node_brk_local(stream, a);
      // ONE collective per hit: every rank's counts, partials and kept keys
      const size_t block = lw_node_block(uint32_t(S), node_cap_);
      st_.node_record_bytes += block;
      collective(0, [&] { comm->all_gather_bytes(nbl_.get(), nball_.get(), block, stream); });
      lw_launch_node_brk_select(stream, a);  // + the report
      st_.kernel_launches += 2;
    });
    node_maxmid_ = maxmid;
    // every rank read the same records: the same next cap, the same collective size
    node_cap_ = lw_node_cap_next(maxmid, uint32_t(nranks));
  } else {
    finish_stage(stream);
    if (!use_brk)
      for (auto& h : m.seg_head) h = kNever;
  }
  if (left) {  // the node radix chain for the series the brackets left (all of them without)
    ++st_.chain_refreshes;
    ChainHooks hooks;
    hooks.before_pass0 = [&] {
      lw_launch_node_predict(stream, a);
      ++st_.kernel_launches;
      collective(1, [&] { comm->all_gather_bytes(pred_local_.get(), pred_all_.get(), S * sizeof(LwPred), stream); });
    };
    hooks.after_pass0 = [&] {
      lw_launch_node_partials(stream, a);
      ++st_.kernel_launches;
      collective(2, [&] {
        comm->all_gather_bytes(agg_local_.get(), agg_all_.get(), S * sizeof(LwPartial), stream);
        comm->all_reduce_sum_u32(hist0_.get<uint32_t>(), hist0_.get<uint32_t>(), S * kB0, stream);
      });
    };
    hooks.after_pass = [&](int k) {
      collective(2 + k, [&] {
        comm->all_reduce_sum_u32(histk_.get<uint32_t>(), histk_.get<uint32_t>(), S * kLongRanks * 256, stream);
      });
    };
    enqueue_chain(stream, a, hooks);
    check(hipGetLastError(), "long-window node launch");
  }
  check(hipEventRecord(m.done.get(), stream), "hipEventRecord");
  check(hipEventRecord(last_done_.get(), stream), "hipEventRecord");
  ++st_.node_refreshes;
  ++st_.refreshes;
}

void LongWindowSet::set_phase_clocks(bool on) {
  Guard g(device_);
  if (on && !dbg_) {
    dbg_ = LwDeviceBuf(std::max<size_t>(1, nseries_) * kBrkQ * 8 * sizeof(unsigned long long), 0);
  } else if (!on && dbg_) {
    if (last_done_) check(hipEventSynchronize(last_done_.get()), "hipEventSynchronize");
    dbg_ = LwDeviceBuf();
  }
}

std::vector<unsigned long long> LongWindowSet::phase_clocks() const {
  std::vector<unsigned long long> v;
  if (!dbg_) return v;
  Guard g(device_);
  v.resize(size_t(nseries_) * kBrkQ * 8);
  if (last_done_) check(hipEventSynchronize(last_done_.get()), "hipEventSynchronize");
  check(hipMemcpy(v.data(), dbg_.get(), v.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost), "hipMemcpy clocks");
  return v;
}

std::vector<std::array<uint32_t, 3>> LongWindowSet::bracket_stats(int mode) const {
  std::vector<std::array<uint32_t, 3>> v;
  for (const auto& x : bracket_state(mode)) v.push_back({x[16], x[17], x[15]});
  return v;
}

// Every series' bracket record of a mode (0 local, 1 node) as its 22 words: lo[3], hi[3],
// delta[3] (float bits), cin[3], valid, hit, refreshes, hits, nounion[3] - reordered
// below to [lo 0-2, hi 3-5, delta 6-8, cin 9-11, valid 12, nounion 13, -, hit 15,
// refreshes 16, hits 17]
std::vector<std::array<uint32_t, 18>> LongWindowSet::bracket_state(int mode) const {
  std::vector<std::array<uint32_t, 18>> v;
  if (mode < 0 || mode > 1 || !bm_[mode].brk) return v;
  Guard g(device_);
  std::vector<LwBrk> b(nseries_);
  if (last_done_) check(hipEventSynchronize(last_done_.get()), "hipEventSynchronize");
  check(hipMemcpy(b.data(), bm_[mode].brk.get(), nseries_ * sizeof(LwBrk), hipMemcpyDeviceToHost), "hipMemcpy brackets");
  for (const auto& x : b) {
    std::array<uint32_t, 18> r{};
    for (int q = 0; q < kBrkQ; ++q) {
      r[q] = x.lo[q];
      r[3 + q] = x.hi[q];
      r[6 + q] = x.delta[q];
      r[9 + q] = x.cin[q];
      r[13] |= x.nounion[q] << q;
    }
    r[12] = x.valid;
    r[15] = x.hit;
    r[16] = x.refreshes;
    r[17] = x.hits;
    v.push_back(r);
  }
  return v;
}

std::vector<double> LongWindowSet::node_collective_us() const {
  std::vector<double> us;
  if (!timed_) return us;
  for (int k = 0; k < kNodeCollectives; ++k) {
    if (!node_timed_[k]) {  // not run this refresh (bracket hit: no chain; no brackets: no record gather)
      us.push_back(std::nan(""));
      continue;
    }
    float ms = 0.f;
    check(hipEventSynchronize(node_events_[2 * k + 1].get()), "hipEventSynchronize");
    check(hipEventElapsedTime(&ms, node_events_[2 * k].get(), node_events_[2 * k + 1].get()), "hipEventElapsedTime");
    us.push_back(double(ms) * 1e3);
  }
  return us;
}

}  // namespace rocmdash
