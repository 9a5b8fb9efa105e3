"""Every window export over the ring states its own test never reaches: one test per scenario of
tests/_window_exports.py. After EVERY refresh of the scenario ``check_all_exports`` holds all
nine exports - export_periods only where the set accepts it, W >= 512 - (and a DeviceWindowSet's
sorted windows) of every ring to the CPU references over a host mirror - several rings at different heads, a ring without rows beside a full one, widths
that take two segments or never get inline rows, lost rows (the 0xFF fill: negative NaNs with a
full payload), unpinned and staged sets, a captured graph, two launches of the exports that
batch by eight rings. The set's own counters are held to the schedule's trace
(test_window_exports_scenarios.py asserts which states that trace reaches), so the path a
scenario is there for is the path that ran."""

import zlib

import numpy as np
import pytest

import _window_exports as we

pytestmark = pytest.mark.gpu


def _push(sc, rings, mirrors, families, rng, step):
    for i, k in enumerate(step):
        if not int(k):
            continue
        t = mirrors[i].head
        if isinstance(k, we.nan_rows):
            x = np.full((int(k), sc.widths[i]), np.nan, np.float32)
        else:
            x = we.ring_rows(rng, families[i], t, int(k), sc.W)
        rings[i].push_many(x, np.arange(t + 1, t + 1 + int(k), dtype=np.uint64))
        mirrors[i].push(x)


def _delta(after, before, keys):
    return {k: after[k] - before[k] for k in keys}


@pytest.mark.parametrize("sc", we.SCENARIOS, ids=lambda sc: sc.name)
def test_exports_over_ring_states(native, cuda, sc):
    import torch

    nat = native
    long = sc.kind == "long"
    try:
        nat.set_pinned_host_rings(sc.pinned)
        nat.set_pull_mode(sc.pull)
        rings = [nat.SeriesRing(w, cap) for w, cap in zip(sc.widths, sc.caps)]
        assert all(r.pinned == sc.pinned for r in rings)
        ws = nat.LongWindowSet(sc.W, 0, use_graph=sc.use_graph) if long else nat.DeviceWindowSet(sc.W, 0)
        assert tuple(ws.add_ring(r) for r in rings) == sc.firsts
        mirrors = [we.Mirror(w) for w in sc.widths]
        families = [we.ring_families(f, w) for f, w in zip(sc.firsts, sc.widths)]
        rng = np.random.default_rng(zlib.crc32(sc.name.encode()))
        bufs = we.ExportBuffers(nat, cuda, sc.widths, sc.W, long)
        out = torch.empty((bufs.S, 8), device=cuda)
        stream = torch.cuda.current_stream().cuda_stream
        keys = (("rows_lost", "ingest_launches", "memcpy_calls", "graph_launches", "refreshes") if long
                else ("launches", "pulled_series", "inline_rows", "memcpy_calls", "refreshes"))
        before = ws.stats()
        for i, (step, rec) in enumerate(zip(sc.steps, we.trace(sc))):
            if step == we.INVALIDATE:
                ws.invalidate()
                continue
            _push(sc, rings, mirrors, families, rng, step)
            if long:
                for m, r in zip(mirrors, rec["rings"]):
                    if r["lost"][1] > r["lost"][0]:
                        m.lose(*r["lost"])
            assert [m.head for m in mirrors] == [r["head"] for r in rec["rings"]] == [r.head for r in rings]
            ws.refresh(out.data_ptr(), stream, *we.PCT)
            we.check_all_exports(ws, mirrors, sc.W, bufs, out, what=f"{sc.name} refresh {i} (+{tuple(int(k) for k in step)})")
            after = ws.stats()
            got = _delta(after, before, keys)
            before = after
            if long:
                want = {"rows_lost": sum(r["lost"][1] - r["lost"][0] for r in rec["rings"]),
                        "ingest_launches": int(rec["ingest"]), "memcpy_calls": rec["memcpy"],
                        "graph_launches": int(sc.use_graph), "refreshes": 1}
            else:
                want = {"launches": rec["launches"], "pulled_series": rec["pulled_series"],
                        "inline_rows": rec["inline_rows"], "memcpy_calls": rec["memcpy"], "refreshes": 1}
            assert got == want, f"{sc.name} refresh {i}: the set's counters moved by {got}, the schedule says {want}"
        st = ws.stats()
        if long:
            assert st["rows_lost"] == sum(m.lost for m in mirrors)
            assert (st["ingest_launches"] == 0) == (not sc.pinned)
        else:
            assert (st["pulled_series"] > 0) == (sc.pinned and sc.pull)
            assert st["inline_rows"] > 0
    finally:
        nat.set_pull_mode(True)
        nat.set_pinned_host_rings(True)
