"""The ring-state scenarios of tests/_window_exports.py, on the CPU: from each schedule alone
(``trace``: a transcription of the host side of LongWindowSet::stage and
DeviceWindowSet::refresh) the states it reaches, and the assertion that the scenarios between
them reach every state test_gpu_window_exports.py is there to cover. The GPU test checks the
sets' own counters against the same traces, so a scenario that stopped reaching a state fails
here, and a set that stopped taking the path fails there."""

import numpy as np
import pytest

import _window_exports as we

LONG = [sc for sc in we.SCENARIOS if sc.kind == "long"]
DEVICE = [sc for sc in we.SCENARIOS if sc.kind == "device"]
SMALL_LONG = [sc for sc in LONG if sc.W == 1024]


def _refreshes(scenarios):
    """(scenario, refresh index, record) of every refresh of the scenarios."""
    return [(sc, i, rec) for sc in scenarios for i, rec in enumerate(we.trace(sc)) if not rec.get("invalidate")]


def test_there_are_about_a_dozen_scenarios_with_distinct_names():
    assert 10 <= len(we.SCENARIOS) <= 14
    assert len(we.BY_NAME) == len(we.SCENARIOS)
    for sc in we.SCENARIOS:
        assert len(sc.widths) == len(sc.caps) and sc.kind in ("long", "device")
        for step in sc.steps:
            assert step == we.INVALIDATE or len(step) == len(sc.widths)


def test_long_scenarios_use_the_smallest_window_but_one():
    assert sorted({sc.W for sc in LONG}) == [1024, 65536]
    big = [sc for sc in LONG if sc.W != 1024]
    assert len(big) == 1 and big[0].caps == (4096, 4096)
    assert all(sc.W <= 1024 for sc in we.SCENARIOS if sc is not big[0])
    for sc in LONG:
        assert len(sc.widths) <= 4 and max(sc.widths) <= 16
        assert all(c & (c - 1) == 0 for c in sc.caps)


def test_long_a_refresh_loses_rows_of_a_push_past_the_host_capacity():
    hits = [(sc.name, i) for sc, i, rec in _refreshes(SMALL_LONG) for r, cap in zip(rec["rings"], sc.caps)
            if cap == 256 and 600 <= r["added"] <= 800 and r["lost"][1] - r["lost"][0] == r["added"] - cap]
    assert hits


def test_long_a_lost_range_crosses_the_device_wrap_in_the_large_scenario():
    sc = we.BY_NAME["long_65536_wrap"]
    crossing = [r["lost"] for rec in we.trace(sc) for r in rec["rings"] if r["crosses_wrap"]]
    assert crossing
    for lo, hi in crossing:
        assert lo < 65536 * (hi // 65536) < hi  # a multiple of W strictly inside


def test_long_a_refresh_loses_rows_on_one_ring_only():
    assert any(sum(r["lost"][1] > r["lost"][0] for r in rec["rings"]) == 1 and len(rec["rings"]) >= 2
               for _, _, rec in _refreshes(SMALL_LONG))


def test_long_a_refresh_leaves_one_ring_s_whole_window_nan():
    # the newest `capacity` rows always survive: a window is all NaN when they are NaN samples
    # themselves (a failing source) on top of the lost rows - both NaN patterns in one window
    hits = [rec for _, _, rec in _refreshes(SMALL_LONG) if any(r["all_nan"] and r["n"] == 1024 for r in rec["rings"])]
    assert hits
    assert any(not all(r["all_nan"] for r in rec["rings"]) for rec in hits)  # beside a ring with samples
    assert any(r["all_nan"] and r["lost"][1] > r["lost"][0] for rec in hits for r in rec["rings"])


def test_long_ring_heads_differ():
    assert any(len({r["head"] for r in rec["rings"]}) > 1 for _, _, rec in _refreshes(SMALL_LONG))


def test_long_a_ring_at_head_0_beside_a_full_window():
    assert any(any(r["head"] == 0 for r in rec["rings"]) and any(r["n"] == sc.W for r in rec["rings"])
               for sc, _, rec in _refreshes(SMALL_LONG))


def test_long_a_refresh_adds_no_rows():
    assert any(rec["rows"] == 0 and i > 0 for _, i, rec in _refreshes(SMALL_LONG))


def test_long_a_small_refresh_takes_the_ingest_kernel_when_pinned_and_copies_when_not():
    pinned, unpinned = we.BY_NAME["long_8_4_lost"], we.BY_NAME["long_8_4_unpinned"]
    assert pinned.pinned and not unpinned.pinned
    assert (pinned.steps, pinned.widths, pinned.caps, pinned.W) == (unpinned.steps, unpinned.widths, unpinned.caps,
                                                                    unpinned.W)
    small = [i for i, rec in enumerate(we.trace(pinned))
             if rec["ingest"] and all(0 < r["added"] <= 100 for r in rec["rings"])]
    assert small
    tu = we.trace(unpinned)
    assert not any(rec["ingest"] for rec in tu)
    for i in small:
        assert tu[i]["memcpy"] >= len(unpinned.widths)
    # a refresh that loses rows never takes the ingest kernel
    for _, _, rec in _refreshes(LONG):
        if any(r["lost"][1] > r["lost"][0] for r in rec["rings"]):
            assert not rec["ingest"]


def test_long_ring_sets_cover_two_segment_widths_and_four_rings():
    widths = {sc.widths for sc in SMALL_LONG}
    assert {(8, 4), (13, 16), (1, 16, 3, 12)} <= widths
    assert all(w > we.LW_SEG_COLS for w in (13, 16))  # streamed as two segments


def test_long_one_scenario_runs_with_a_graph_as_well():
    graph = [sc for sc in LONG if sc.use_graph]
    assert len(graph) == 1
    twin = [sc for sc in LONG if not sc.use_graph and (sc.steps, sc.widths, sc.caps, sc.W, sc.pinned)
            == (graph[0].steps, graph[0].widths, graph[0].caps, graph[0].W, graph[0].pinned)]
    assert len(twin) == 1


def test_device_windows_and_variants():
    assert sorted({sc.W for sc in DEVICE}) == [64, 512]
    for W in (64, 512):
        pull = [sc for sc in DEVICE if sc.W == W and sc.pinned and sc.pull]
        staged = [sc for sc in DEVICE if sc.W == W and sc.pinned and not sc.pull]
        assert len(pull) == 1 and len(staged) == 1 and pull[0].steps == staged[0].steps
        tp, ts = we.trace(pull[0]), we.trace(staged[0])
        assert sum(r["pulled_series"] for r in tp if not r["invalidate"]) > 0
        assert sum(r["inline_rows"] for r in tp if not r["invalidate"]) > 0
        assert sum(r["pulled_series"] for r in ts if not r["invalidate"]) == 0
        assert sum(r["memcpy"] for r in ts if not r["invalidate"]) > sum(r["memcpy"] for r in tp if not r["invalidate"])
    unpinned = [sc for sc in DEVICE if not sc.pinned]
    assert len(unpinned) == 1
    assert sum(r["pulled_series"] for r in we.trace(unpinned[0]) if not r["invalidate"]) == 0


@pytest.mark.parametrize("sc", DEVICE, ids=lambda sc: sc.name)
def test_device_scenario_reaches_the_states(sc):
    W = sc.W
    assert sc.widths == (11, 5, 1, 16, 17, 3, 4, 8, 2, 7)
    assert all(c % (2 * W) == 0 for c in sc.caps)
    tr = we.trace(sc)
    refreshes = [rec for rec in tr if not rec["invalidate"]]
    # ten rings: three stats launches a refresh, two launches for the exports that batch by 8
    assert all(rec["launches"] == 3 for rec in refreshes)
    assert -(-len(sc.widths) // we.MAX_RINGS_PER_LAUNCH) == 3 and -(-len(sc.widths) // we.EXPORT_RINGS_PER_LAUNCH) == 2
    # the device ring of 2 W rows wraps at least twice, for every ring
    assert all(r["wraps"] >= 2 for r in refreshes[-1]["rings"])
    # rings advance by different amounts in one refresh
    assert any({1, 4, 5, 9, 0} <= {r["added"] for r in rec["rings"]} for rec in refreshes)
    # one ring stays at head 0 for the first refreshes, beside filled ones
    assert all(rec["rings"][-1]["head"] == 0 and rec["rings"][0]["n"] == W for rec in refreshes[:3])
    assert refreshes[-1]["rings"][-1]["n"] == W
    # a 257-row step and a 3 W step: both fall back to a full sort
    for rows in (257, 3 * W):
        hit = [rec for rec in refreshes if all(r["added"] == rows for r in rec["rings"])]
        assert hit and not any(r["incremental"] for r in hit[0]["rings"])
    # 255 and 256 rows stay incremental where the 2 W-deep device ring still holds the leaving rows
    for rows in (255, 256):
        hit = [rec for rec in refreshes if all(r["added"] == rows for r in rec["rings"])]
        assert hit and all(r["incremental"] == (rows <= W) for r in hit[0]["rings"])
    # invalidate() in the middle, followed by a refresh that sorts again
    at = [i for i, rec in enumerate(tr) if rec["invalidate"]]
    assert len(at) == 1 and 2 < at[0] < len(tr) - 3
    assert not any(r["incremental"] for r in tr[at[0] + 1]["rings"])
    # the width-17 ring never gets inline rows; the others do when pinned or not
    wide = sc.widths.index(17)
    assert all(rec["rings"][wide]["inline"] == 0 for rec in refreshes)
    assert any(rec["rings"][sc.widths.index(1)]["inline"] > 0 for rec in refreshes)
    if sc.pinned and sc.pull:
        assert any(rec["rings"][wide]["pulled"] for rec in refreshes)
        assert any(r["pulled"] and r["inline"] == we.INLINE_ROWS for rec in refreshes for r in rec["rings"])
    else:
        assert not any(r["pulled"] for rec in refreshes for r in rec["rings"])
        assert any(rec["rings"][wide]["staged"] and rec["rings"][wide]["incremental"] for rec in refreshes)
        assert any(r["staged"] and r["inline"] == we.INLINE_ROWS for rec in refreshes for r in rec["rings"])


def test_host_rings_hold_every_push_of_a_device_scenario():
    # DeviceWindowSet has no lost rows: a push never exceeds the host ring
    for sc in DEVICE:
        for step in sc.steps:
            if step != we.INVALIDATE:
                assert all(int(k) <= cap for k, cap in zip(step, sc.caps))


def test_mirror_and_input_columns():
    m = we.Mirror(3)
    rows, head = m.window(8)
    assert rows.shape == (0, 3) and head == 0
    rng = np.random.default_rng(1)
    fam = we.ring_families(12, 3)
    assert fam[-1] == "odd_nan" and we.ring_families(5, 1) == ["boundary"]
    x = we.ring_rows(rng, fam, 0, 4000, 64)
    m.push(x)
    m.lose(10, 20)
    rows, head = m.window(64)
    assert head == 4000 and rows.shape == (64, 3) and m.lost == 10
    assert np.isnan(m.rows[10:20]).all()
    bits = x[:, -1].view(np.uint32)[np.isnan(x[:, -1])]
    assert set(bits.tolist()) == set(we.ODD_NANS.tolist())  # every pattern, and no other
    assert all((b & 0x7FC00000) == 0x7FC00000 for b in bits.tolist())  # quiet, none signalling
    assert 0 < len(bits) < 4000


def test_export_parameters_are_what_every_export_accepts():
    from rocmdash.ops.window_autocorr import check_autocorr, check_scale
    from rocmdash.ops.window_buckets import check_bounds
    from rocmdash.ops.window_excursions import check_thresholds
    from rocmdash.ops.window_joint import check_joint_bounds

    S = 74
    b = we.export_bounds(S)
    assert b.shape == (S, we.B) and b.dtype == np.float32
    check_bounds(b, S)
    check_joint_bounds(b, S)
    check_thresholds(np.ascontiguousarray(b[:, [5, 10]]), S)
    assert len({tuple(np.round(np.diff(r) / np.diff(r)[0], 3)) for r in b[:6]}) > 1  # unevenly spaced
    for W in (64, 512, 1024, 65536):
        check_autocorr(we.L, we.autocorr_span(W), W)
    check_scale((np.float32(4095.0 / 200.0) * (1 + np.arange(S) % 3)).astype(np.float32), S)
