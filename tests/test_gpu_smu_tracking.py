"""SMU table publication tracking (csrc/sources.h SmuTableTracker) on the real amd-smi
source: two SmiSources, one with ROCMDASH_SMU_TABLE_TRACK=0, each polled for ~1 s by a
free-running native Sampler while the GPU alternates between busy and idle (so the
table's values move)."""

import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RUN_S = 1.0
TABLE_COLS = [0, 1, 2, 5, 6, 7]  # temperatures, gfx activity, socket power, umc activity: from the table


def _raw_source(nat):
    """An SmiSource on the raw SMU-table path (a start-up calibration refused by a busy
    box is retried on sampling, here every second - as tests/test_gpu.py does)."""
    src = nat.make_smi_source(0, 0)
    t_end = time.monotonic() + 30.0
    while src.counts()["raw_path"] != 1 and time.monotonic() < t_end:
        src.sample()
        time.sleep(0.05)
    c = src.counts()
    assert c["raw_path"] == 1, (src.info()["metrics_calibration"], c)
    return src


def _poll(nat, src, torch):
    """RUN_S of free-running sampling under a 100 ms busy / 100 ms idle GPU load; returns
    (counts before, counts just before stop, counts after stop, rows, timestamps)."""
    ring = nat.SeriesRing(src.width, 1 << 17)
    smp = nat.Sampler(src, ring, 10.0)
    a = torch.randn(4096, 4096, device="cuda", dtype=torch.bfloat16)
    torch.cuda.synchronize()
    c0 = src.counts()
    smp.start_free(50000.0)
    t_end = time.perf_counter() + RUN_S
    while time.perf_counter() < t_end:
        t_busy = time.perf_counter() + 0.1
        while time.perf_counter() < min(t_busy, t_end):
            (a @ a).sum().item()
        time.sleep(max(0.0, min(0.1, t_end - time.perf_counter())))
    c1 = src.counts()
    smp.stop()
    c2 = src.counts()
    rows, ts = ring.window(int(ring.head))
    return c0, c1, c2, rows, ts


def test_tracked_source_reads_the_table_only_around_publications(native, monkeypatch):
    import torch

    nat = native
    monkeypatch.setenv("ROCMDASH_SMI_RECALIBRATE_S", "1")
    monkeypatch.delenv("ROCMDASH_SMU_TABLE_MIN_US", raising=False)
    monkeypatch.delenv("ROCMDASH_SMU_TABLE_TRACK", raising=False)
    tracked = _raw_source(nat)
    monkeypatch.setenv("ROCMDASH_SMU_TABLE_TRACK", "0")
    plain = _raw_source(nat)
    assert tracked.counts()["table_track_enabled"] == 1 and plain.counts()["table_track_enabled"] == 0

    # direct reads: no hint, every sample reads the table
    r0 = tracked.counts()["raw_reads"]
    for _ in range(20):
        assert tracked.sample() is not None
    c = tracked.counts()
    assert c["raw_reads"] - r0 == 20 and c["table_track"] == 0 and c["table_skips"] == 0

    p0, p1, p2, prow, _ = _poll(nat, plain, torch)
    t0, t1, t2, trow, tts = _poll(nat, tracked, torch)

    def d(a, b, k):
        return b[k] - a[k]

    pubs_plain, pubs_tracked = d(p0, p2, "raw_table_changes"), d(t0, t2, "raw_table_changes")
    reads_plain, reads_tracked = d(p0, p2, "raw_reads"), d(t0, t2, "raw_reads")
    print(f"untracked: {len(prow)} rows, {reads_plain:.0f} table reads, {pubs_plain:.0f} publications; "
          f"tracked: {len(trow)} rows, {reads_tracked:.0f} table reads, {pubs_tracked:.0f} publications, "
          f"skips {d(t0, t2, 'table_skips'):.0f}, period {t1['table_period_us']:.1f} us, locks {t2['table_locks']:.0f}, "
          f"resyncs {t2['table_resyncs']:.0f}, missed {t2['table_missed']:.0f}")
    assert p1["table_track"] == 0 and d(p0, p2, "table_skips") == 0 and reads_plain == len(prow)
    assert t1["table_track"] == 2, t1  # locked while polled
    assert t2["table_track"] == 0  # the hint left with the sampler thread
    assert abs(t1["table_period_us"] - 20000.0) < 1000.0, t1
    assert abs(pubs_tracked - pubs_plain) <= 2, (pubs_tracked, pubs_plain)
    assert t2["table_missed"] == 0
    assert reads_tracked <= reads_plain / 4, (reads_tracked, reads_plain)
    assert len(trow) > len(prow)
    assert t2["raw_misses"] == 0 and p2["raw_misses"] == 0
    assert reads_tracked + d(t0, t2, "table_skips") == len(trow)

    # A row taken right after a detected change carries that read's table values: every
    # row whose table columns differ from the row before came from a sample that read the
    # table - it lasted a table read (>= 43 us; the next row starts then), not the 20 us
    # between the starts of samples that repeat the last table.
    tab = trow[:, TABLE_COLS]
    same = np.all((tab[1:] == tab[:-1]) | (np.isnan(tab[1:]) & np.isnan(tab[:-1])), axis=1)
    moved = np.flatnonzero(~same) + 1
    moved = moved[moved < len(trow) - 1]
    assert len(moved) >= 3, "the busy / idle load moved the table's values"
    assert len(moved) <= pubs_tracked + 1
    took_us = (tts[moved + 1].astype(np.int64) - tts[moved].astype(np.int64)) / 1e3
    print("samples whose table values moved took (us):", np.round(np.sort(took_us)[:5], 1), "...", len(moved))
    assert took_us.min() > 35.0, took_us.min()

    # back to direct reads: every sample reads again
    r0 = tracked.counts()["raw_reads"]
    for _ in range(10):
        tracked.sample()
    assert tracked.counts()["raw_reads"] - r0 == 10
