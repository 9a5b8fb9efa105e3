"""Window quantile trend on the CPU: the numpy reference against the exact oracle of
tests/_exact.py, the geometry's edges, the argument rules, the kernels' compile-time resources,
the agent without a device, the figure, the exporter's /quantiles document and the page's charts."""

import json
import math
import os
import re
import shutil
import subprocess
import urllib.error
import urllib.request

import numpy as np
import pytest

import _exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_BYTES_PER_CU = 160 * 1024
PCT = (50.0, 90.0, 99.0)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _assert_reference(got, rows, head, W, P, pct, nonfinite_ok=()):
    """The rules of tests/test_gpu_window_quantiles.py::_assert_quantiles, for the reference."""
    from rocmdash.ops.window_trend import trend_geometry

    n, S = rows.shape
    assert got.dtype == np.float32 and got.shape == (S, P + 1, 4)
    _, ranges = trend_geometry(head, n, W, P)
    first, made = head - n, 0
    for j, (b, e) in enumerate(ranges):
        g = got[:, j]
        if e <= b:
            assert (g[:, 3] == 0).all() and np.isnan(g[:, :3]).all(), (j, g)
            continue
        ex = _exact.exact_stats(np.ascontiguousarray(rows[b - first:e - first]), pct)
        np.testing.assert_array_equal(g[:, 3], ex.count.astype(np.float32))
        for s in range(S):
            for q in range(3):
                have, where = g[s, q], f"slot {j} series {s} q {q}"
                if not ex.nv[s]:
                    assert np.isnan(have), where
                elif ex.frac[s, q] == 0 or ex.x0[s, q] == ex.x1[s, q]:
                    assert _exact._same(have, ex.x0[s, q]), where
                elif not (np.isfinite(ex.x0[s, q]) and np.isfinite(ex.x1[s, q])):
                    assert s in nonfinite_ok, where
                    continue
                else:
                    assert _exact._within_one_ulp(have, ex.percentile[s, q]), (where, have, ex.percentile[s, q])
                    assert ex.x0[s, q] <= have <= ex.x1[s, q], where
                made += 1
    return made


# ---- reference --------------------------------------------------------------------------
@pytest.mark.parametrize("pct", [PCT, (0.0, 37.5, 100.0)])
@pytest.mark.parametrize("head_off", [0, 1, 77])
@pytest.mark.parametrize("n,W,P", [(1, 64, 8), (63, 64, 64), (64, 64, 8), (300, 512, 8), (512, 512, 64)])
def test_reference_against_the_exact_oracle(n, W, P, head_off, pct):
    from rocmdash.ops.window_quantiles import window_quantiles_reference

    rng = np.random.default_rng(n + P)
    rows = _exact.family_rows(rng, 0, n, W, width=len(_exact.FAMILIES), blips=(n // 2,))
    ends = rng.normal(0, 1, (n, 1)).astype(np.float32)
    ends[0], ends[-1] = -np.inf, np.inf
    rows = np.concatenate([rows, ends], axis=1)
    S = rows.shape[1]
    head = n + head_off
    got = window_quantiles_reference(rows, head, W, P, pct)
    nonfinite = (_exact.INF_SERIES, S - 1)
    made = _assert_reference(got, rows, head, W, P, pct, nonfinite)
    c = W // P
    slots = (head - 1) // c - (head - n) // c + 1
    assert made >= slots * 3 * (S - len(nonfinite))
    F = _exact.FAMILIES.index
    assert (got[F("all_nan"), :, 3] == 0).all() and np.isnan(got[F("all_nan"), :, :3]).all()
    full = got[F("constant"), :, 3] > 0
    assert (got[F("constant")][full][:, :3] == 42.0).all()


def test_reference_of_signed_zeroes_is_zero():
    """-0.0 sorts below +0.0, but the interpolation (x0 + (x1 - x0) * frac, as the stats kernels
    do it) does not keep a zero's sign: the values are zero, of either sign."""
    from rocmdash.ops.window_quantiles import window_quantiles_reference

    rows = np.array([[0.0], [-0.0]] * 32, np.float32)  # 8 rows per column: four -0.0, four +0.0
    got = window_quantiles_reference(rows, 64, 64, 8, (0.0, 100.0, 40.0))
    assert (got[0, 1:, 3] == 8).all() and (got[0, 0, 3] == 0)
    assert (got[0, 1:, :3] == 0).all() and np.isnan(got[0, 0, :3]).all()


# ---- geometry edges ---------------------------------------------------------------------
def test_fewer_rows_than_a_column_and_an_unaligned_head():
    from rocmdash.ops.window_quantiles import window_quantiles_reference

    W, P = 64, 8  # c = 8
    x = np.arange(5, dtype=np.float32).reshape(5, 1)
    got = window_quantiles_reference(x, 5, W, P, PCT)  # n < c: one slot, the newest
    assert (got[0, :P, 3] == 0).all() and np.isnan(got[0, :P, :3]).all()
    np.testing.assert_array_equal(got[0, P], np.array([2.0, 3.6, 3.96, 5], np.float32))
    got = window_quantiles_reference(x, 11, W, P, PCT)  # rows 6 .. 10: two in column 0, three in column 1
    assert (got[0, :, 3] == [0] * (P - 1) + [2, 3]).all()
    np.testing.assert_array_equal(got[0, P - 1, :3], np.array([0.5, 0.9, 0.99], np.float32))
    np.testing.assert_array_equal(got[0, P, :3], np.array([3.0, 3.8, 3.98], np.float32))
    got = window_quantiles_reference(np.zeros((0, 3), np.float32), 0, W, P, PCT)
    assert got.shape == (3, P + 1, 4) and (got[:, :, 3] == 0).all() and np.isnan(got[:, :, :3]).all()


def test_argument_rules():
    from rocmdash.ops.window_quantiles import check_pct, window_quantiles_reference

    assert check_pct((0, 50, 100)) == (0.0, 50.0, 100.0)
    for bad in ((50.0, float("nan"), 99.0), (50.0, 90.0, 100.5), (-1.0, 50.0, 99.0), (50.0, 90.0), (1, 2, float("inf"))):
        with pytest.raises(ValueError):
            check_pct(bad)
    rows = np.zeros((64, 2), np.float32)
    for P, W in ((6, 64), (128, 64), (0, 64), (8, 96)):
        with pytest.raises(ValueError):
            window_quantiles_reference(rows, 64, W, P)
    with pytest.raises(ValueError):
        window_quantiles_reference(rows, 63, 64, 8)  # more rows than the head has seen
    with pytest.raises(ValueError):
        window_quantiles_reference(rows, 64, 64, 8, (50.0, 90.0, 101.0))


# ---- kernel resources -------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_quantile_kernels_have_no_scratch_and_fit_lds(tmp_path):
    """The flags and the rules of tests/test_kernel_resources.py, for the quantile kernels."""
    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", "window_quantiles.hip"), "-o", str(tmp_path / "k.o"),
         "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600,
    )
    assert res.returncode == 0, res.stderr[-3000:]
    kernels, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs): (\d+)", line)
        if m and name is not None:
            kernels[name][m.group(1)] = int(m.group(2))
    assert len(kernels) >= 2, res.stderr[-2000:]  # the LDS sort (per number of waves) and the radix select
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert r.get("LDS Size [bytes/block]", 0) <= LDS_BYTES_PER_CU, (k, r)


# ---- agent without a device -------------------------------------------------------------
def _cpu_agent(window=128):
    from rocmdash.config import SamplerConfig
    from rocmdash.runtime.agent import GpuAgent

    return GpuAgent(0, source="synthetic", counters="synthetic", cfg=SamplerConfig(window=window, ring_capacity=4 * window),
                    use_gpu=False)


def test_cpu_agent_window_quantiles(native):
    from rocmdash.ops.window_quantiles import window_quantiles_reference

    agent = _cpu_agent(128)
    try:
        assert agent.dws is None
        empty = agent.window_quantiles(8).numpy()
        assert (empty[:, :, 3] == 0).all() and np.isnan(empty[:, :, :3]).all()
        agent.prefill(150)
        got = agent.window_quantiles(8).numpy()
        trend = agent.window_trend(8).numpy()
        assert got.shape == (len(agent.series), 9, 4) and got.dtype == np.float32
        s = 0
        for i, r in enumerate(agent.rings):
            rows, _ = agent.window_host(i)
            want = window_quantiles_reference(rows, r.head, 128, 8, agent.pct)
            np.testing.assert_array_equal(_bits(got[s:s + r.width]), _bits(want))
            assert _assert_reference(got[s:s + r.width], rows, r.head, 128, 8, agent.pct) > 0
            s += r.width
        np.testing.assert_array_equal(_bits(got[:, :, 3]), _bits(trend[:, :, 3]))
        has = trend[:, :, 3] > 0
        for q in range(3):
            assert (got[:, :, q][has] >= trend[:, :, 0][has]).all() and (got[:, :, q][has] <= trend[:, :, 1][has]).all()
        with pytest.raises(ValueError):
            agent.window_quantiles(6)
        with pytest.raises(ValueError):
            agent.window_quantiles(256)
    finally:
        agent.close()


# ---- figure -----------------------------------------------------------------------------
_AGE = [30.0, 20.0, float("nan"), 10.0, 0.0]
_P50 = [1.0, 2.0, float("nan"), 1.5, 0.5]
_P90 = [2.0, 3.0, float("nan"), 2.5, 1.5]
_P99 = [4.0, 5.0, float("nan"), 4.5, 3.5]


def test_create_quantiles_json_shape():
    from rocmdash.viz.figures import create_quantiles

    fig = create_quantiles("Temperature", _AGE, (50, 90, 99.9), (np.array(_P50, np.float32), _P90, _P99), 100, 220)
    doc = json.loads(fig.to_json())  # strict JSON: no NaN
    assert [t["name"] for t in doc["data"]] == ["p50", "p90", "p99.9"]
    for t, y in zip(doc["data"], (_P50, _P90, _P99)):
        assert t["type"] == "scatter" and t["mode"] == "lines" and "connectgaps" not in t and "fill" not in t
        assert t["x"] == [-30.0, -20.0, None, -10.0, 0.0]
        assert t["y"] == [y[0], y[1], None, y[3], y[4]]
    assert len({t["line"]["color"] for t in doc["data"]}) == 3
    assert doc["layout"]["yaxis"]["range"] == [0, 100] and doc["layout"]["height"] == 220
    assert doc["layout"]["xaxis"]["title"]["text"] == "seconds"
    # a slot with an age but no valid sample is a gap too; no max_val: autorange
    doc = json.loads(create_quantiles("t", [2.0, 1.0, 0.0], PCT, ([1, float("nan"), 1],) * 3).to_json())
    assert doc["data"][2]["y"] == [1, None, 1] and doc["data"][2]["x"] == [-2.0, -1.0, 0.0] and doc["layout"]["yaxis"] == {}


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

    cfg = SamplerConfig(window=64, ring_capacity=256, smi_hz=200, counter_hz=400)
    src = LocalNodeSource(devices=[0], source="synthetic", counters="synthetic", cfg=cfg, **kw)
    src.agents[0].stop()  # the background samplers: rows are pushed from this thread only
    return src


def test_exporter_serves_quantiles_json_and_404_without(native, monkeypatch):
    """A synthetic source without a GPU: /quantiles is the documented JSON with null for NaN;
    off (the default) it is a 404 with a hint; the quantiles never reach /metrics."""
    import torch

    from rocmdash.prom.exporter import Exporter

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # agents on the CPU, wherever this runs
    monkeypatch.delenv("ROCMDASH_WINDOW_QUANTILES", raising=False)
    src = _local_source(window_quantiles=8)
    exp = Exporter(src, hostname="n1")
    try:
        agent = src.agents[0]
        assert agent.dws is None
        agent.prefill(40)  # the window is not full: the oldest slots are empty
        exp.serve("127.0.0.1", 0)
        code, ctype, body = _get(exp.port, "/quantiles")
        assert code == 200 and ctype == "application/json"
        assert b"NaN" not in body
        doc = json.loads(body)
        assert doc["columns"] == 8 and doc["series"] == list(src.series) and list(doc["gpus"]) == [agent.info.gpu_id]
        assert doc["percentiles"] == [50.0, 90.0, 99.0]
        assert len(doc["age_rows"]) == 9 and doc["age_rows"][-1] == 0 and doc["age_rows"][0] is None
        per = doc["gpus"][agent.info.gpu_id]
        assert set(per) == set(src.series)
        want = agent.window_quantiles(8).numpy()
        for s, metric in enumerate(src.series):
            m = per[metric]
            assert list(m) == ["p50", "p90", "p99", "count"]
            for i, k in enumerate(m):
                assert len(m[k]) == 9
                for v, w in zip(m[k], want[s, :, i]):
                    assert (v is None and math.isnan(w)) or v == float(w)
            assert m["count"][0] == 0 and m["p50"][0] is None
        assert 40 <= sum(per[src.series[0]]["count"]) == agent.rings[0].head < 56
        metrics = _get(exp.port, "/metrics")[2].decode()
        assert "quantile" not in metrics.replace("quantile=", "")  # (a summary's own label, if any, is not this)
        assert _get(exp.port, "/trend")[0] == 404  # the trend is its own option
    finally:
        exp.close()

    src = _local_source()
    exp = Exporter(src, hostname="n1")
    try:
        assert src.quantile_columns is None
        exp.serve("127.0.0.1", 0)
        code, _, body = _get(exp.port, "/quantiles")
        assert code == 404 and b"--window-quantiles" in body
        assert _get(exp.port, "/metrics")[0] == 200
    finally:
        exp.close()


def test_metrics_and_trend_are_byte_identical_with_the_quantiles_on_and_off(native):
    """The same seeded snapshot with and without a quantile trend renders the same /metrics
    text and the same /trend document."""
    import copy

    from rocmdash.prom.exporter import SyntheticSource, render_quantiles, render_trend
    from rocmdash.prom.exposition import render_snapshot

    snap, _ = SyntheticSource(2, seed=3).collect()
    snap.window_series = tuple(snap.columns[:3])
    snap.window = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    snap.window_trend = np.full((2, 3, 9, 4), 1.5, np.float32)
    snap.window_trend_age_rows = np.array([np.nan] + list(range(7, -1, -1)), np.float64)
    off, trend_off = render_snapshot(snap, hostname="n1"), render_trend(snap)
    assert render_quantiles(snap) is None
    on = copy.copy(snap)
    on.window_quantiles = np.full((2, 3, 9, 4), np.nan, np.float32)
    on.window_quantiles[:, :, 1:, :] = 2.5
    on.window_quantiles[:, :, 0, 3] = 0
    on.window_quantiles_age_rows = np.array([np.nan] + list(range(7, -1, -1)), np.float64)
    on.window_quantiles_pct = (50.0, 99.9, 100.0)
    assert render_snapshot(on, hostname="n1") == off
    assert render_trend(on) == trend_off
    body = render_quantiles(on)
    assert "NaN" not in body
    doc = json.loads(body)
    assert doc["columns"] == 8 and doc["percentiles"] == [50.0, 99.9, 100.0]
    assert doc["age_rows"][0] is None and doc["age_rows"][-1] == 0
    m = doc["gpus"][snap.gpu_ids[0]][snap.window_series[0]]
    assert list(m) == ["p50", "p99.9", "p100", "count"]
    assert m["p99.9"] == [None] + [2.5] * 8 and m["count"] == [0.0] + [2.5] * 8


def test_exporter_option_is_checked_before_the_samplers_start(native, monkeypatch):
    import torch

    from rocmdash.runtime.agent import GpuAgent

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCMDASH_WINDOW_QUANTILES", "16")
    src = _local_source()
    try:
        assert src.quantile_columns == 16
        src.agents[0].prefill(70)
        snap, _ = src.collect()
        assert snap.window_quantiles.shape == (1, len(src.series), 17, 4) and snap.window_quantiles_age_rows.shape == (17,)
        assert snap.window_quantiles_pct == (50.0, 90.0, 99.0)
        assert getattr(snap, "window_trend", None) is None
    finally:
        src.close()
    started = []
    monkeypatch.setattr(GpuAgent, "start", lambda self: started.append(self))
    monkeypatch.setattr(GpuAgent, "__init__", lambda self, *a, **k: started.append(self))
    monkeypatch.setenv("ROCMDASH_WINDOW_QUANTILES", "6")
    with pytest.raises(ValueError):
        _local_source()
    monkeypatch.delenv("ROCMDASH_WINDOW_QUANTILES")
    for bad in (6, 128, 2048):  # no power of two; more columns than the window's 64 rows; too many
        with pytest.raises(ValueError):
            _local_source(window_quantiles=bad)
    assert not started  # no agent was made, no sampler started


def test_exporter_flag_parses(monkeypatch):
    from rocmdash.prom import exporter

    seen = {}

    class Stop(Exception):
        pass

    def fake_source(**kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(exporter, "LocalNodeSource", fake_source)
    with pytest.raises(Stop):
        exporter.main(["--window-quantiles", "32", "--source", "synthetic"])
    assert seen["window_quantiles"] == 32 and seen["window_trend"] is None


# ---- page -------------------------------------------------------------------------------
def test_page_quantile_figures_only_with_quantiles():
    from rocmdash.prom.exporter import SyntheticSource
    from rocmdash.ui.page import window_quantile_figures, window_trend_figures
    from rocmdash.viz.panels import POWER, TEMP, UTIL

    snap, _ = SyntheticSource(2, seed=1).collect()
    assert window_quantile_figures(snap, snap.gpu_ids) is None  # none carried: the page is as it was
    snap.window_series = (UTIL, TEMP, POWER, "amd_gpu_gfx_clock")
    snap.window_quantiles = np.full((2, 4, 9, 4), 1.0, np.float32)
    snap.window_quantiles[:, :, 0] = np.nan
    snap.window_quantiles_age_rows = np.array([np.nan] + list(range(70, -1, -10)), np.float64)
    snap.window_quantiles_pct = (50.0, 90.0, 99.0)
    assert window_trend_figures(snap, snap.gpu_ids) is None
    figs = window_quantile_figures(snap, [snap.gpu_ids[1]])
    assert [k for k, _ in figs] == [f"plot_quantiles_{m}_{snap.gpu_ids[1]}_" for m in ("gpu_util", "temp", "power")]
    doc = json.loads(figs[0][1].to_json())
    assert [t["name"] for t in doc["data"]] == ["p50", "p90", "p99"]
    assert doc["data"][2]["y"] == [None] + [1.0] * 8 and doc["data"][2]["x"][0] is None and doc["data"][2]["x"][-1] == 0
