"""Window period trend (rocmdash.ops.window_periods) without a GPU: the reference against a
triple loop in Python ints, the options' limits, the reference's identities, the period per slot,
the exporter's /periods, the figure, the page and the agent's CPU path."""

import json
import urllib.error
import urllib.request

import numpy as np
import pytest

from _window_periods import rows as _rows, scale as _scale


# ---- reference --------------------------------------------------------------------------
def _brute(rows, scale, head, P, L, span):
    """The semantics as a loop over (slot, k, t) in Python ints: slot j is column
    (head - 1) // c - P + j cut to the newest min(n, span) rows; pairs stay inside the slot."""
    from rocmdash.ops.window_autocorr import quantise

    n, S = rows.shape
    q, v = quantise(rows, scale)
    q, v = q.tolist(), v.tolist()
    c, first, lo = span // P, head - n, head - min(n, span)
    out = [[[[0] * 4 for _ in range(L + 1)] for _ in range(P + 1)] for _ in range(S)]
    for j in range(P + 1):
        col = (head - 1) // c - P + j
        b, e = max(col * c, lo), min((col + 1) * c, head)
        if col < 0 or b >= e or n == 0:
            continue
        for s in range(S):
            for k in range(L + 1):
                for r in range(b, e - k):
                    t, u = r - first, r + k - first
                    out[s][j][k][0] += v[t][s] * v[u][s]
                    out[s][j][k][1] += q[t][s] * v[u][s]
                    out[s][j][k][2] += v[t][s] * q[u][s]
                    out[s][j][k][3] += q[t][s] * q[u][s]
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("n,head", [(512, 512), (512, 3 * 512 + 17), (300, 2 * 512 + 100), (700, 5 * 512 + 63), (0, 0)])
def test_reference_against_a_triple_loop(n, head):
    from rocmdash.ops.window_periods import window_periods_reference

    span, P, L, W = 512, 8, 5, 1024
    x = _rows(n + head, 2, n, nan=0.05).T
    got = window_periods_reference(x, _scale(2), head, W, P, L, span)
    assert got.dtype == np.int64 and got.shape == (2, P + 1, L + 1, 4)
    np.testing.assert_array_equal(got, _brute(x, _scale(2), head, P, L, span))


def test_options_limits_and_refusals():
    from rocmdash.ops.window_periods import check_periods, parse_periods

    ok = [(8, 255, 1 << 16, 1 << 16), (64, 255, 1 << 16, 1 << 20), (8, 32, 512, 512), (64, 1, 4096, 4096),
          (16, 1023, 1 << 20, 1 << 20), (16, 1, 1 << 20, 1 << 26), (8, 1024, 1 << 14, 1 << 14), (64, 255, 1 << 16, None)]
    for P, L, span, W in ok:
        assert check_periods(P, L, span, W) == (P, L, span)
    assert check_periods(8, None, None, 4096) == (8, 255, 4096)  # the defaults: 255 lags, min(W, 65536)
    assert check_periods(64, None, None, 1 << 20) == (64, 255, 1 << 16)
    assert check_periods(64, 255) == (64, 255, 1 << 16)
    bad = {"columns": [(4, 8, 512, 512), (128, 8, 1 << 16, 1 << 16), (12, 8, 4096, 4096)],
           "rows per column": [(16, 8, 512, 512), (8, 8, 1 << 20, 1 << 20)],
           "lags": [(8, 0, 4096, 4096), (8, 1025, 1 << 16, 1 << 16), (8, 33, 512, 512), (64, 513, 1 << 16, 1 << 16)],
           "at most 16384": [(64, 256, 1 << 16, 1 << 16), (16, 1024, 1 << 16, 1 << 16)],
           "window": [(8, 8, 1024, 512)],
           "power of two": [(8, 8, 768, 1024), (8, 8, 256, 1024), (8, 8, 1 << 21, 1 << 22)],
           "integers": [(8.5, 8, 512, 512), (8, "x", 512, 512), (True, 8, 512, 512)]}
    for word, cases in bad.items():
        for P, L, span, W in cases:
            with pytest.raises(ValueError, match=word):
                check_periods(P, L, span, W)
    assert parse_periods("8", 4096) == (8, 255, 4096)
    assert parse_periods(" 16/100 ", 1 << 16) == (16, 100, 1 << 16)
    assert parse_periods("8/32/512", 4096) == (8, 32, 512) == parse_periods((8, 32, 512), 4096)
    assert parse_periods(64) == (64, 255, 1 << 16) and parse_periods((8, 16), 512) == (8, 16, 512)
    for spec in ("", "x", "8/", "8/16/512/1", "8/1.5", None, 8.0, "4", "8/33/512", "8/16/1024"):
        with pytest.raises(ValueError):
            parse_periods(spec, 512)


def test_constants_agree_with_the_headers():
    import os
    import re

    from rocmdash.ops import window_autocorr as wa, window_periods as wp

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "csrc", "window_periods.h")).read() + open(os.path.join(root, "csrc", "window_periods_plan.h")).read()

    def const(name):
        m = re.search(rf"constexpr uint32_t {name} = (?:1u << (\d+)|(\d+));", text)
        assert m, f"{name} is no plain integer constant any more"
        return 1 << int(m.group(1)) if m.group(1) else int(m.group(2))

    want = {"kMinPeriodsSpan": wp.MIN_SPAN, "kMinPeriodsColumns": wp.MIN_COLUMNS, "kMaxPeriodsColumns": wp.MAX_COLUMNS,
            "kMinPeriodsRowsPerColumn": wp.MIN_ROWS_PER_COLUMN, "kMaxPeriodsRowsPerColumn": wp.MAX_ROWS_PER_COLUMN,
            "kMaxPeriodsWords": wp.MAX_WORDS, "kPeriodsChunk": wa.CHUNK, "kPeriodsSeriesGroup": wa.SERIES_GROUP,
            "kPeriodsLagBlock": wa.LAG_BLOCK}
    assert {k: const(k) for k in want} == want
    assert wp.quantise is wa.quantise and wp.check_scale is wa.check_scale and wp.default_scale is wa.default_scale
    assert wp.correlogram is wa.correlogram and wp.pick_period is wa.pick_period and wp.MAX_SPAN == wa.MAX_SPAN
    assert wp.DEFAULT_LAGS == wa.LAG_BLOCK - 1 and wp.MAX_COLUMNS * (wp.DEFAULT_LAGS + 1) == wp.MAX_WORDS


def test_reference_identities():
    from rocmdash.ops.window_autocorr import window_autocorr_reference
    from rocmdash.ops.window_periods import periods_age_rows, periods_geometry, window_periods_reference
    from rocmdash.ops.window_trend import trend_age_rows, trend_geometry

    span, P, L, W = 1024, 8, 40, 2048
    c = span // P
    S, n = 3, 1500
    x = _rows(7, S, n + 200, nan=0.03).T
    sc = _scale(S)
    for head in (n, 4 * W + 5, 4 * W + c - 1, 9 * W):
        rows = x[:n]
        out = window_periods_reference(rows, sc, head, W, P, L, span)
        newest = rows[n - span:]
        np.testing.assert_array_equal(out[:, :, 0, 0].sum(axis=1), np.count_nonzero(~np.isnan(newest), axis=0))
        whole = window_autocorr_reference(rows, sc, L, span)
        np.testing.assert_array_equal(out[:, :, 0, 3].sum(axis=1), whole[:, 0, 3])
        _, ranges = periods_geometry(head, n, P, span)
        np.testing.assert_array_equal(ranges, trend_geometry(head, span, span, P)[1])
        np.testing.assert_array_equal(periods_age_rows(head, n, P, span), trend_age_rows(head, span, span, P))
        assert (out[:, :, :, 0] <= np.maximum((ranges[:, 1] - ranges[:, 0])[None, :, None] - np.arange(L + 1)[None, None], 0)).all()
    # span == W: the trend's own slots
    np.testing.assert_array_equal(periods_geometry(5000, 2048, P, W)[1], trend_geometry(5000, 2048, W, P)[1])
    # a full column's block does not change while the head advances inside the same newest column
    head = 6 * W + 3
    base = window_periods_reference(x[:n], sc, head, W, P, L, span)
    _, r0 = periods_geometry(head, n, P, span)
    for step in (1, 17, c - 4):
        out = window_periods_reference(x[step:n + step], sc, head + step, W, P, L, span)
        _, r1 = periods_geometry(head + step, n, P, span)
        assert (head + step - 1) // c == (head - 1) // c
        for j in range(P + 1):
            if r1[j, 1] - r1[j, 0] == c:
                assert (r0[j] == r1[j]).all()
                np.testing.assert_array_equal(out[:, j], base[:, j])
        assert not np.array_equal(out[:, P], base[:, P]) and not np.array_equal(out[:, 0], base[:, 0])


# ---- period per slot --------------------------------------------------------------------
def _two_periods():
    """[n, 2]: series 0 a square wave of period 9 in the first half and 13 in the second; series 1
    the same with one column constant and one all NaN."""
    span = 4096
    t = np.arange(span)
    wave = np.where(t < span // 2, np.where(t % 9 < 5, 80.0, 20.0), np.where(t % 13 < 7, 80.0, 20.0)).astype(np.float32)
    other = wave.copy()
    other[512:1024] = 50.0
    other[3072:3584] = np.nan
    return np.stack([wave, other], axis=1)


def test_slot_periods_follow_a_period_change():
    from rocmdash.ops.window_periods import slot_periods, window_periods_reference

    span, P, L = 4096, 8, 64
    sums = window_periods_reference(_two_periods(), _scale(2), span, span, P, L, span)
    period, strength, valid = slot_periods(sums)
    assert period.shape == strength.shape == valid.shape == (2, P + 1) and valid.dtype == np.int64
    nan = float("nan")
    # head is a multiple of the column: slot 0 is the empty column before the rows
    np.testing.assert_array_equal(period[0], [nan, 9, 9, 9, 9, 13, 13, 13, 13])
    np.testing.assert_array_equal(period[1], [nan, 9, nan, 9, 9, 13, 13, nan, 13])
    assert np.isnan(strength[0, 0]) and (strength[0, 1:] > 0.9).all()
    np.testing.assert_array_equal(np.isnan(strength), np.isnan(period))
    assert valid[0].tolist() == [0] + [512] * 8 and valid[1].tolist() == [0, 512, 512, 512, 512, 512, 512, 0, 512]
    with pytest.raises(ValueError):
        slot_periods(sums[0])


# ---- figure -----------------------------------------------------------------------------
def test_create_periods_json():
    from rocmdash.viz.figures import create_periods

    nan = float("nan")
    fig = create_periods("GPU 0: power", [nan, 30.0, 20.0, 10.0, 0.0], [nan, 9.0, nan, 13.0, 13.0], [nan, 0.5, nan, 0.75, 1.0])
    doc = json.loads(fig.to_json())
    (tr,) = doc["data"]
    assert tr["type"] == "scatter" and tr["mode"] == "lines+markers" and tr["connectgaps"] is False
    assert tr["x"] == [None, -30.0, -20.0, -10.0, 0.0] and tr["y"] == [None, 9.0, None, 13.0, 13.0]
    assert tr["text"] == [None, "strength 0.50", None, "strength 0.75", "strength 1.00"]
    assert tr["marker"]["opacity"] == [1.0, 0.25, 1.0, 0.625, 1.0]
    assert doc["layout"]["xaxis"]["title"]["text"] == "seconds" and doc["layout"]["yaxis"]["title"]["text"] == "period (samples)"
    assert json.loads(fig.to_plotly().to_json()) == doc
    bare = json.loads(create_periods("t", [1.0, 0.0], [7, None]).to_json())
    assert bare["data"][0]["y"] == [7, None] and bare["data"][0]["text"] == [None, None]


# ---- exporter ---------------------------------------------------------------------------
def _get(port, path):
    try:
        with urllib.request.urlopen(f"http://127.0.0.1:{port}{path}", timeout=10) as r:
            return r.status, r.headers.get("Content-Type"), r.read()
    except urllib.error.HTTPError as e:
        return e.code, e.headers.get("Content-Type"), e.read()


def _local_source(**kw):
    from rocmdash.config import SamplerConfig
    from rocmdash.prom.exporter import LocalNodeSource

    cfg = SamplerConfig(window=512, ring_capacity=2048, smi_hz=200, counter_hz=400)
    src = LocalNodeSource(devices=[0], source="synthetic", counters="synthetic", cfg=cfg, **kw)
    src.agents[0].stop()  # the background samplers: rows are pushed from this thread only
    return src


def _strict(body):
    def no_constant(name):
        raise AssertionError(f"{name} in a strict JSON document")

    return json.loads(body, parse_constant=no_constant)


def test_exporter_serves_periods_json_and_404_without(native, monkeypatch):
    """A synthetic source without a GPU: /periods is the documented strict JSON with null for "no
    period" and for an empty slot's age; off (the default) it is a 404 with a hint, the snapshot
    carries nothing and /metrics has nothing new."""
    import torch

    from rocmdash.ops.window_periods import periods_age_rows, slot_periods, window_periods_reference
    from rocmdash.prom.exporter import Exporter
    from rocmdash.prom.exposition import render_snapshot

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # agents on the CPU, wherever this runs
    monkeypatch.delenv("ROCMDASH_WINDOW_PERIODS", raising=False)
    src = _local_source(window_periods="8/16")
    exp = Exporter(src, hostname="n1")
    try:
        agent = src.agents[0]
        assert agent.dws is None and src.periods == (8, 16, 512)
        agent.prefill(300)  # fewer rows than the span: the oldest slots are empty
        exp.serve("127.0.0.1", 0)
        code, ctype, body = _get(exp.port, "/periods?x=1")
        assert code == 200 and ctype == "application/json"
        doc = _strict(body)
        assert set(doc) == {"columns", "lags", "span", "age_rows", "series", "gpus"}
        assert doc["columns"] == 8 and doc["lags"] == 16 and doc["span"] == 512 and doc["series"] == list(src.series)
        head = int(agent.rings[0].head)
        age = periods_age_rows(head, min(head, 512), 8, 512)
        assert doc["age_rows"] == [None if a != a else float(a) for a in age] and None in doc["age_rows"] and doc["age_rows"][-1] == 0
        assert list(doc["gpus"]) == [agent.info.gpu_id]
        per = doc["gpus"][agent.info.gpu_id]
        want = agent.window_periods(8, 16, 512, src.periods_scale).numpy()
        assert want.shape == (len(src.series), 9, 17, 4) and want.dtype == np.int64
        s = 0
        for i, r in enumerate(agent.rings):  # the CPU path is the reference over each ring's window
            rows = np.asarray(agent.window_host(i)[0], np.float32).reshape(-1, r.width)
            ref = window_periods_reference(rows, src.periods_scale[s:s + r.width], int(r.head), 512, 8, 16, 512)
            np.testing.assert_array_equal(want[s:s + r.width], ref)
            s += r.width
        period, strength, valid = slot_periods(want)
        assert list(per) == list(src.series)
        for s, m in enumerate(src.series):
            d = per[m]
            assert set(d) == {"period_samples", "strength", "rows"}
            assert d["rows"] == valid[s].tolist() and all(isinstance(v, int) for v in d["rows"])
            assert d["period_samples"] == [None if v != v else int(v) for v in period[s]]
            assert d["strength"] == [None if v != v else float(v) for v in strength[s]]
            assert d["period_samples"][0] is None and d["rows"][0] == 0  # an empty slot
        assert _get(exp.port, "/autocorr")[0] == 404
        snap, _ = src.collect()
        assert snap.window_periods.shape == (1, len(src.series), 9, 17, 4) and snap.window_periods_span == 512
        assert len(snap.window_periods_age_rows) == 9
        on = render_snapshot(snap, hostname="n1")
        snap.window_periods = snap.window_periods_span = snap.window_periods_age_rows = None
        assert render_snapshot(snap, hostname="n1") == on  # nothing of it in /metrics
    finally:
        exp.close()

    src = _local_source()
    exp = Exporter(src, hostname="n1")
    try:
        assert src.periods is None and src.periods_scale is None
        exp.serve("127.0.0.1", 0)
        code, _, body = _get(exp.port, "/periods")
        assert code == 404 and b"--window-periods" in body
        snap, _ = src.collect()
        assert snap.window_periods is None and snap.window_periods_span is None and snap.window_periods_age_rows is None
    finally:
        exp.close()


def test_exporter_option_from_the_environment_and_refusals(native, monkeypatch, capsys):
    import torch

    from rocmdash.prom.exporter import main

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCMDASH_WINDOW_PERIODS", "8/32/512")
    src = _local_source()
    try:
        assert src.periods == (8, 32, 512)
        src.agents[0].prefill(600)
        snap, _ = src.collect()
        assert snap.window_periods.shape == (1, len(src.series), 9, 33, 4) and snap.window_periods.dtype == np.int64
        assert int(snap.window_periods[0, 0, :, 0, 0].sum()) == 512
    finally:
        src.close()
    started = []
    monkeypatch.setattr("rocmdash.runtime.agent.GpuAgent.start", lambda self: started.append(self))
    # the default 255 lags need columns of 510 rows; a span beyond the window of 512
    for bad in ("8", "4/8", "8/33", "16/8", "8/8/1024", "8/8/768", "abc", "8/8/512/1"):
        monkeypatch.setenv("ROCMDASH_WINDOW_PERIODS", bad)
        with pytest.raises(ValueError):
            _local_source()
    assert not started  # refused before any sampler started
    monkeypatch.delenv("ROCMDASH_WINDOW_PERIODS")
    for bad in ("4", "8/0", "8/x", "64", "8/8/100", "128/8"):
        with pytest.raises(SystemExit):
            main(["--window-periods", bad])
        assert "--window-periods" in capsys.readouterr().err
    assert not started


# ---- page -------------------------------------------------------------------------------
def test_page_periods_figures_only_with_sums():
    from rocmdash.ops.window_periods import periods_age_rows, window_periods_reference
    from rocmdash.prom.exporter import SyntheticSource, render_periods
    from rocmdash.ui.page import window_periods_figures
    from rocmdash.viz.panels import POWER, TEMP

    snap, _ = SyntheticSource(2, seed=1).collect()
    assert window_periods_figures(snap, snap.gpu_ids) is None and render_periods(snap) is None  # the page is as it was
    snap.window_series = (POWER, TEMP)
    sums = window_periods_reference(_two_periods(), _scale(2), 4096, 4096, 8, 64, 4096)
    snap.window_periods, snap.window_periods_span = np.stack([sums, sums]), 4096
    snap.window_periods_age_rows = periods_age_rows(4096, 4096, 8, 4096)
    figs = window_periods_figures(snap, [snap.gpu_ids[1]])
    g = snap.gpu_ids[1]
    assert [k for k, _ in figs] == [f"plot_periods_temp_{g}_", f"plot_periods_power_{g}_"]
    temp, power = (json.loads(f.to_json())["data"][0] for _, f in figs)
    assert power["y"] == [None, 9, 9, 9, 9, 13, 13, 13, 13] and temp["y"] == [None, 9, None, 9, 9, 13, 13, None, 13]
    assert power["x"][0] is None and power["x"][-1] == 0 and power["x"][1] < power["x"][2] < 0
    doc = json.loads(render_periods(snap))
    assert doc["gpus"][g][POWER]["period_samples"] == [None, 9, 9, 9, 9, 13, 13, 13, 13]
    assert doc["age_rows"] == [None, 3584.0, 3072.0, 2560.0, 2048.0, 1536.0, 1024.0, 512.0, 0.0]
