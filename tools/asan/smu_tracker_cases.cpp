// SmuTableTracker (csrc/sources.h) on a simulated clock, the cases of
// tests/test_smu_table_tracker.py as a stand-alone program for
// -fsanitize=address,undefined (host code only):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Icsrc tools/asan/smu_tracker_cases.cpp -o smu_tracker_cases && ./smu_tracker_cases
//
// Prints one line per case and "failed=<n>"; exit status 1 if any case failed.
#include <cstdint>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "sources.h"

using rocmdash::SmuTableTracker;

namespace {
constexpr int64_t kReadNs = 50000, kSkipNs = 20000;
int g_failed = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ok = false;                                                          \
    }                                                                      \
  } while (0)

std::vector<int64_t> publications(const std::vector<std::pair<double, int>>& periods_ms, int64_t jitter_ns, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_int_distribution<int64_t> jit(-jitter_ns, jitter_ns);
  std::vector<int64_t> out;
  int64_t t = 3000000;
  for (const auto& pc : periods_ms)
    for (int i = 0; i < pc.second; ++i) {
      out.push_back(t);
      t += int64_t(pc.first * 1e6) + (jitter_ns ? jit(rng) : 0);
    }
  return out;
}

struct Detection {
  size_t k;
  int64_t latency;
  size_t jump, reads;
  int state;
};

struct Sim {
  SmuTableTracker& t;
  std::vector<int64_t> pubs;
  bool use_fw_ts;
  int64_t now = 0;
  size_t seen = 0, reads = 0, samples = 0, reads_since = 0;
  std::vector<Detection> det;
  Sim(SmuTableTracker& tr, std::vector<int64_t> p, bool fw, bool hint = true) : t(tr), pubs(std::move(p)), use_fw_ts(fw) {
    t.set_back_to_back(hint);
  }
  void run_until(int64_t end) {
    while (now < end) {
      ++samples;
      if (!t.should_read(now)) {
        now += kSkipNs;
        continue;
      }
      ++reads;
      ++reads_since;
      const int state = int(t.state());
      size_t n = seen;
      while (n < pubs.size() && pubs[n] <= now + kReadNs / 2) ++n;
      const bool changed = n != seen;
      const uint64_t fw_ts = (use_fw_ts && n) ? uint64_t(pubs[n - 1] / 10) : 0;
      t.record(now, changed, fw_ts);
      if (changed) {
        det.push_back({n - 1, now - pubs[n - 1], n - seen, reads_since, state});
        reads_since = 0;
        seen = n;
      }
      now += kReadNs;
    }
  }
};

int64_t jitter() {
  const int64_t j = (rocmdash::kSmuGuardNs - 2 * kReadNs) / 2;
  return j < rocmdash::kSmuGuardNs * 2 / 5 ? j : rocmdash::kSmuGuardNs * 2 / 5;
}

bool steady(bool fw) {
  bool ok = true;
  SmuTableTracker t(rocmdash::kSmuGuardNs, rocmdash::kSmuHardNs);
  const auto pubs = publications({{20, 120}}, jitter(), 1);
  Sim s(t, pubs, fw);
  s.run_until(pubs.back() + 1000000);
  CHECK(s.det.size() == pubs.size());
  size_t first = s.det.size();
  for (size_t i = 0; i < s.det.size(); ++i)
    if (s.det[i].state == SmuTableTracker::kLocked) {
      first = i;
      break;
    }
  CHECK(first <= 6);
  const size_t window = size_t(2 * t.guard_ns() / kReadNs + 2);
  for (size_t i = first; i < s.det.size(); ++i) {
    CHECK(s.det[i].state == SmuTableTracker::kLocked);
    CHECK(s.det[i].jump == 1);
    CHECK(s.det[i].latency + kReadNs / 2 >= 0 && s.det[i].latency + kReadNs / 2 <= kReadNs);
    CHECK(s.det[i].reads <= window);
  }
  CHECK(t.missed() == 0 && t.resyncs() == 0 && t.locks() == 1);
  CHECK(s.reads < s.samples / 8);
  return ok;
}

bool cadence(bool fw, double new_ms) {
  bool ok = true;
  SmuTableTracker t(rocmdash::kSmuGuardNs, rocmdash::kSmuHardNs);
  const size_t n_old = 40;
  const auto pubs = publications({{20, int(n_old)}, {new_ms, 40}}, jitter(), 2 + unsigned(new_ms));
  Sim s(t, pubs, fw);
  s.run_until(pubs.back() + 1000000);
  CHECK(t.resyncs() >= 1 && t.locks() >= 2);
  CHECK(t.state() == SmuTableTracker::kLocked);
  const int64_t dp = t.period_ns() - int64_t(new_ms * 1e6);
  CHECK(dp <= t.guard_ns() && -dp <= t.guard_ns());
  size_t relock = 0;
  for (size_t i = 0; i < s.det.size(); ++i)
    if (s.det[i].state != SmuTableTracker::kLocked) relock = i + 1;
  CHECK(relock < s.det.size() && s.det[relock].k <= n_old + 12);
  size_t lost = 0;
  for (const Detection& d : s.det) {
    lost += d.jump - 1;
    if (relock < s.det.size() && (d.k < n_old || d.k >= s.det[relock].k)) CHECK(d.jump == 1);
  }
  CHECK(lost <= 3 && t.missed() <= 3);
  CHECK(s.reads <= size_t(s.now / kReadNs) + 1);
  return ok;
}

bool stall() {
  bool ok = true;
  SmuTableTracker t(rocmdash::kSmuGuardNs, rocmdash::kSmuHardNs);
  auto pubs = publications({{20, 30}}, jitter(), 5);
  Sim s(t, pubs, true);
  s.run_until(pubs.back() + 1000000);
  CHECK(t.state() == SmuTableTracker::kLocked);
  const size_t reads0 = s.reads, samples0 = s.samples;
  s.run_until(pubs.back() + 1000000000);
  CHECK(t.state() == SmuTableTracker::kAcquire && t.resyncs() == 1);
  CHECK(s.reads - reads0 + size_t(20000000 / kSkipNs + 10) >= s.samples - samples0);
  const int64_t back = s.now + 5000000;
  for (int i = 0; i < 12; ++i) s.pubs.push_back(back + 20000000ll * i);
  s.run_until(s.pubs.back() + 1000000);
  CHECK(t.state() == SmuTableTracker::kLocked && t.locks() == 2);
  return ok;
}

bool hard_bound() {
  bool ok = true;
  SmuTableTracker t(rocmdash::kSmuGuardNs, rocmdash::kSmuHardNs);
  const auto pubs = publications({{200, 8}}, 0, 6);
  Sim s(t, pubs, true);
  int64_t last_read = 0, gap = 0;
  while (s.now < pubs.back()) {
    const size_t before = s.reads;
    s.run_until(s.now + 1);
    if (s.reads != before) {
      if (s.now - last_read > gap) gap = s.now - last_read;
      last_read = s.now;
    }
  }
  CHECK(t.state() == SmuTableTracker::kLocked);
  CHECK(gap <= t.hard_ns() + kReadNs + kSkipNs);
  return ok;
}

bool no_hint() {
  bool ok = true;
  const auto pubs = publications({{20, 30}}, 0, 7);
  SmuTableTracker t(rocmdash::kSmuGuardNs, rocmdash::kSmuHardNs);
  Sim s(t, pubs, true, false);
  s.run_until(pubs.back());
  CHECK(s.reads == s.samples && t.state() == SmuTableTracker::kOff && t.locks() == 0);
  SmuTableTracker u(rocmdash::kSmuGuardNs, rocmdash::kSmuHardNs);
  Sim v(u, pubs, true);
  v.run_until(pubs[15]);
  CHECK(u.state() == SmuTableTracker::kLocked);
  u.set_back_to_back(false);
  const size_t reads0 = v.reads, samples0 = v.samples;
  v.run_until(pubs.back());
  CHECK(u.state() == SmuTableTracker::kOff && v.reads - reads0 == v.samples - samples0);
  return ok;
}

void report(const char* name, bool ok) {
  std::printf("%s: %s\n", name, ok ? "ok" : "FAILED");
  g_failed += !ok;
}
}  // namespace

int main() {
  report("steady fw_ts", steady(true));
  report("steady host_clock", steady(false));
  report("cadence 20->10 fw_ts", cadence(true, 10));
  report("cadence 20->10 host_clock", cadence(false, 10));
  report("cadence 20->100 fw_ts", cadence(true, 100));
  report("cadence 20->100 host_clock", cadence(false, 100));
  report("stall", stall());
  report("hard bound", hard_bound());
  report("no hint", no_hint());
  std::printf("failed=%d\n", g_failed);
  return g_failed ? 1 : 0;
}
