"""SmuTableTracker (csrc/sources.h) through its binding, on a simulated clock: the
firmware publishes a table every ~20 ms, a back-to-back sampler asks every 20 us (table
skipped) or 50 us (table read). The tracker must lock onto the publications, read only
around them, and lose nothing - also when the cadence changes or stops.

tools/asan/smu_tracker_cases.cpp runs the same cases as a stand-alone C++ program under
-fsanitize=address,undefined (test_tracker_cases_are_sanitizer_clean)."""

import os
import random
import shutil
import subprocess

import pytest

from rocmdash.runtime import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ_NS = 50_000  # a sample that reads the table
SKIP_NS = 20_000  # a sample that repeats it (the 50 kHz free-running cap)
OFF, ACQUIRE, LOCKED = 0, 1, 2


@pytest.fixture(scope="module")
def nat():
    return native.load()


def publications(periods_ms, jitter_ns, seed):
    """Publication times (ns): for each (period_ms, count) that many intervals of
    period + U(-jitter, jitter), starting at 3 ms."""
    rng = random.Random(seed)
    t, out = 3_000_000, []
    for period_ms, count in periods_ms:
        for _ in range(count):
            out.append(t)
            t += int(period_ms * 1e6) + rng.randint(-jitter_ns, jitter_ns)
    return out


class Sim:
    """Drives a tracker the way SmiSource::sample does. Per publication index k it keeps
    the latency of the read that saw it (read start - publication time, ns), the table
    reads since the previous detection and the tracker's state at the detection."""

    def __init__(self, tracker, pubs, use_fw_ts, hint=True):
        self.t, self.pubs, self.use_fw_ts = tracker, pubs, use_fw_ts
        self.now = 0
        self.seen = 0  # publications the last read had seen
        self.reads = self.samples = 0
        self.reads_since = 0
        self.det = []  # (k, latency_ns, jump, reads_since, state_before)
        self.t.set_back_to_back(hint)

    def visible(self, at):
        n = self.seen
        while n < len(self.pubs) and self.pubs[n] <= at:
            n += 1
        return n

    def run_until(self, end_ns):
        while self.now < end_ns:
            self.samples += 1
            if not self.t.should_read(self.now):
                self.now += SKIP_NS
                continue
            self.reads += 1
            self.reads_since += 1
            state = self.t.state
            n = self.visible(self.now + READ_NS // 2)  # the mailbox answers mid-read
            changed = n != self.seen
            fw_ts = self.pubs[n - 1] // 10 if (self.use_fw_ts and n) else 0
            self.t.record(self.now, changed, fw_ts)
            if changed:
                self.det.append((n - 1, self.now - self.pubs[n - 1], n - self.seen, self.reads_since, state))
                self.reads_since = 0
                self.seen = n
            self.now += READ_NS


def jitter_for(nat):
    # An interval differs from the tracker's period estimate (a running mean of earlier
    # intervals, itself within the jitter) by at most 2 x jitter, and host-clock intervals
    # carry up to one read of detection latency at either end: 2 J + 2 reads <= guard.
    j = (nat.SMU_GUARD_NS - 2 * READ_NS) // 2
    assert j > 0
    return min(j, int(0.4 * nat.SMU_GUARD_NS))


@pytest.mark.parametrize("use_fw_ts", [True, False], ids=["fw_ts", "host_clock"])
def test_locks_and_reads_only_around_publications(nat, use_fw_ts):
    t = nat.SmuTableTracker()
    guard = t.guard_ns
    pubs = publications([(20, 120)], jitter_for(nat), seed=1)
    s = Sim(t, pubs, use_fw_ts)
    s.run_until(pubs[-1] + 1_000_000)
    assert len(s.det) == len(pubs), "every publication is seen"
    first_locked = next(k for k, _, _, _, st in s.det if st == LOCKED)
    assert first_locked <= 6, f"locked only at publication {first_locked}"
    assert t.state == LOCKED and abs(t.period_ns - 20_000_000) <= guard
    window_reads = 2 * guard // READ_NS + 2  # the polled window's worth
    for k, lat, jump, reads, st in s.det[first_locked:]:
        assert st == LOCKED, (k, st)
        assert jump == 1, f"publication {k - 1} missed"
        assert 0 <= lat + READ_NS // 2 <= READ_NS, f"publication {k} seen {lat} ns after it, not by the first read"
        assert reads <= window_reads, (k, reads)
    assert t.missed == 0 and t.resyncs == 0 and t.locks == 1
    # what it is for: a small fraction of the samples read the table
    locked_reads = sum(r for _, _, _, r, st in s.det[first_locked:])
    assert locked_reads / (len(pubs) - first_locked) < window_reads
    assert s.reads < s.samples / 8


@pytest.mark.parametrize("use_fw_ts", [True, False], ids=["fw_ts", "host_clock"])
@pytest.mark.parametrize("new_ms", [10, 100])
def test_cadence_change_resyncs(nat, use_fw_ts, new_ms):
    t = nat.SmuTableTracker()
    guard = t.guard_ns
    n_old, n_new = 40, 40
    pubs = publications([(20, n_old), (new_ms, n_new)], jitter_for(nat), seed=2 + new_ms)
    s = Sim(t, pubs, use_fw_ts)
    s.run_until(pubs[-1] + 1_000_000)
    assert t.resyncs >= 1 and t.locks >= 2
    assert t.state == LOCKED and abs(t.period_ns - new_ms * 1_000_000) <= guard
    # publications are lost only while the change is being noticed: none before the last
    # old-cadence one, none once locked again
    relock = next(i for i in range(len(s.det) - 1, -1, -1) if s.det[i][4] != LOCKED) + 1
    assert s.det[relock][0] <= n_old + 12, "locked onto the new cadence within a handful of publications"
    for k, lat, jump, reads, st in s.det:
        if k < n_old or k >= s.det[relock][0]:
            assert jump == 1, f"publication {k - 1} missed outside the change"
    assert sum(j - 1 for _, _, j, _, _ in s.det) <= 3
    assert t.missed <= 3
    assert s.reads <= s.now // READ_NS + 1  # never more than the every-sample rate


def test_stall_falls_back_to_acquire(nat):
    t = nat.SmuTableTracker()
    pubs = publications([(20, 30)], jitter_for(nat), seed=5)
    s = Sim(t, pubs, True)
    s.run_until(pubs[-1] + 1_000_000)
    assert t.state == LOCKED
    reads0, samples0 = s.reads, s.samples
    s.run_until(pubs[-1] + 1_000_000_000)  # nothing published for 1 s
    assert t.state == ACQUIRE and t.resyncs == 1
    # after the window closed every sample reads again
    assert s.reads - reads0 >= (s.samples - samples0) - (20_000_000 // SKIP_NS + 10)
    # and it locks again when the publications come back
    more = [s.now + 5_000_000 + 20_000_000 * i for i in range(12)]
    s.pubs = pubs + more
    s.run_until(more[-1] + 1_000_000)
    assert t.state == LOCKED and t.locks == 2


def test_hard_bound_without_a_read(nat):
    """Locked on a slow cadence the table is still read every hard_ns."""
    t = nat.SmuTableTracker()
    pubs = publications([(200, 8)], 0, seed=6)
    s = Sim(t, pubs, True)
    last_read, gap = 0, 0
    while s.now < pubs[-1]:
        before = s.reads
        s.run_until(s.now + 1)
        if s.reads != before:
            gap = max(gap, s.now - last_read)
            last_read = s.now
    assert t.state == LOCKED
    assert gap <= t.hard_ns + READ_NS + SKIP_NS


def test_without_the_hint_every_sample_reads(nat):
    t = nat.SmuTableTracker()
    pubs = publications([(20, 30)], 0, seed=7)
    s = Sim(t, pubs, True, hint=False)
    s.run_until(pubs[-1])
    assert s.reads == s.samples and t.state == OFF and t.locks == 0
    # the hint taken away while locked: back to every sample at once
    u = nat.SmuTableTracker()
    s = Sim(u, pubs, True)
    s.run_until(pubs[15])
    assert u.state == LOCKED
    u.set_back_to_back(False)
    reads0, samples0 = s.reads, s.samples
    s.run_until(pubs[-1])
    assert u.state == OFF and s.reads - reads0 == s.samples - samples0


def test_tracker_cases_are_sanitizer_clean(tmp_path):
    """The same cases as a stand-alone program with AddressSanitizer and UBSan."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "smu_tracker_cases"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{ROOT}/csrc", f"{ROOT}/tools/asan/smu_tracker_cases.cpp", "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "failed=0" in run.stdout, run.stdout
