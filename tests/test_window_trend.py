"""Window trend on the CPU: the geometry (rocmdash.ops.window_trend.trend_geometry is the one
statement of the semantics), the numpy reference against a brute-force per-slot loop, the
argument rules, the kernels' compile-time resources, the agent without a device, the figure,
the exporter's /trend document and the page's charts."""

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


# ---- geometry ---------------------------------------------------------------------------
@pytest.mark.parametrize("P", [8, 64])
@pytest.mark.parametrize("W", [64, 4096])
def test_geometry_partitions_the_window_into_aligned_columns(W, P):
    from rocmdash.ops.window_trend import trend_age_rows, trend_geometry

    c = W // P
    for base in (W, 5 * W):
        for rem in sorted({0, 1 % c, c - 1}):
            head = base + rem
            for n in (0, 1, W - 1, W):
                got_c, r = trend_geometry(head, n, W, P)
                assert got_c == c and r.shape == (P + 1, 2) and r.dtype == np.int64
                full = r[r[:, 1] > r[:, 0]]
                if n == 0:
                    assert len(full) == 0
                    continue
                # the slots partition [head - n, head) exactly, in order
                assert full[0, 0] == head - n and full[-1, 1] == head
                assert (full[1:, 0] == full[:-1, 1]).all()
                # every slot lies inside one aligned column, the one its index names
                last = (head - 1) // c
                for j, (b, e) in enumerate(r):
                    if e > b:
                        assert b // c == (e - 1) // c == last - P + j
                    else:
                        assert b == e == 0
                # slot 0 is empty exactly when the window starts on a column boundary and is full
                if n == W:  # a full window: slot 0 is empty exactly when it starts on a column boundary
                    assert (r[0, 1] == r[0, 0]) == ((head - n) % c == 0)
                assert r[P, 0] <= head - 1 < r[P, 1]  # the newest slot holds the newest row
                age = trend_age_rows(head, n, W, P)
                assert age[P] == 0 and np.isnan(age).sum() == P + 1 - len(full)
                assert (np.diff(age[~np.isnan(age)]) < 0).all()


def test_geometry_rejects_windows_that_do_not_exist():
    from rocmdash.ops.window_trend import trend_geometry

    for head, n in ((3, 4), (100, 65), (10, -1)):
        with pytest.raises(ValueError):
            trend_geometry(head, n, 64, 8)


def test_check_columns():
    from rocmdash.ops.window_trend import check_columns

    assert check_columns(8, 64) == 8 and check_columns(64, 64) == 1
    assert check_columns(256, 1 << 24) == 65536 and check_columns(1024, 1 << 26) == 65536
    for P, W in ((0, 64), (6, 64), (2048, 4096), (128, 64), (128, 1 << 24), (512, 1 << 26), (8, 96)):
        with pytest.raises(ValueError):
            check_columns(P, W)


# ---- reference --------------------------------------------------------------------------
def _brute_force(rows, head, W, P):
    """Row by row: every row goes to the slot of its absolute column."""
    n, S = rows.shape
    c = W // P
    last = (head - 1) // c
    out = np.full((S, P + 1, 4), np.nan, np.float32)
    out[:, :, 3] = 0
    for s in range(S):
        slots = [[] for _ in range(P + 1)]
        for i in range(n):
            x = rows[i, s]
            if not math.isnan(x):
                slots[(head - n + i) // c - (last - P)].append(x)
        for j, v in enumerate(slots):
            if v:
                keys = _exact.fkey(np.array(v, np.float32))
                total = sum((np.longdouble(x) for x in v), np.longdouble(0))
                with np.errstate(invalid="ignore", over="ignore"):
                    out[s, j] = (v[int(np.argmin(keys))], v[int(np.argmax(keys))], np.float32(np.float64(total / len(v))), len(v))
    return out


@pytest.mark.parametrize("head_off", [0, 1, 77])
@pytest.mark.parametrize("n,W,P", [(1, 64, 8), (63, 64, 64), (64, 64, 8), (300, 512, 8), (512, 512, 64)])
def test_reference_against_a_per_row_loop(n, W, P, head_off):
    from rocmdash.ops.window_trend import window_trend_reference

    rng = np.random.default_rng(n + P)
    rows = _exact.family_rows(rng, 0, n, W, width=len(_exact.FAMILIES), blips=(n // 2,))
    ends = rng.normal(0, 1, (n, 1)).astype(np.float32)
    ends[0], ends[-1] = -np.inf, np.inf
    rows = np.concatenate([rows, ends], axis=1)
    head = n + head_off
    with np.errstate(invalid="ignore"):
        got, want = window_trend_reference(rows, head, W, P), _brute_force(rows, head, W, P)
    assert got.dtype == np.float32 and got.shape == (rows.shape[1], P + 1, 4)
    np.testing.assert_array_equal(got.view(np.uint32)[:, :, [0, 1, 3]], want.view(np.uint32)[:, :, [0, 1, 3]])
    np.testing.assert_array_equal(got[:, :, 2], want[:, :, 2])  # NaN == NaN here
    F = _exact.FAMILIES.index
    assert (got[F("all_nan"), :, 3] == 0).all() and np.isnan(got[F("all_nan"), :, :3]).all()
    z = got[F("zeroes")]
    if n >= 64:  # -0.0 and +0.0 are told apart somewhere
        zr = rows[:, F("zeroes")]
        assert (np.signbit(z[:, 0]) & (z[:, 0] == 0)).any() == bool(((zr == 0) & np.signbit(zr)).any() and (z[:, 0] == 0).any())
    if n > 1:  # +inf and -inf: ordinary values for min / max, IEEE for the mean
        assert np.isneginf(got[-1, :, 0]).any() and np.isposinf(got[-1, :, 1]).any()


def test_reference_mean_of_opposite_infinities_is_nan():
    from rocmdash.ops.window_trend import window_trend_reference

    rows = np.array([[np.inf], [-np.inf], [1.0], [np.nan]] * 16, np.float32)  # 64 rows, 8 per column
    with np.errstate(invalid="ignore"):
        got = window_trend_reference(rows, 64, 64, 8)
    assert np.isnan(got[0, 1:, 2]).all() and (got[0, 1:, 3] == 6).all()
    assert np.isneginf(got[0, 1:, 0]).all() and np.isposinf(got[0, 1:, 1]).all()


# ---- kernel resources -------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src", ["window_trend.hip"])
def test_trend_kernels_have_no_scratch_and_fit_lds(src, tmp_path):
    """The flags and the rules of tests/test_kernel_resources.py, for the trend's kernels."""
    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", src), "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    assert len(kernels) >= 2, res.stderr[-2000:]  # a wave per slot, a workgroup per slot
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert r.get("LDS Size [bytes/block]", 0) <= LDS_BYTES_PER_CU, (k, r)


# ---- agent without a device -------------------------------------------------------------
def _cpu_agent(window=128):
    from rocmdash.config import SamplerConfig
    from rocmdash.runtime.agent import GpuAgent

    return GpuAgent(0, source="synthetic", counters="synthetic", cfg=SamplerConfig(window=window, ring_capacity=4 * window),
                    use_gpu=False)


def test_cpu_agent_window_trend(native):
    from rocmdash.ops.window_trend import trend_age_rows, window_trend_reference

    agent = _cpu_agent(128)
    try:
        assert agent.dws is None
        empty = agent.window_trend(8).numpy()
        assert (empty[:, :, 3] == 0).all() and np.isnan(empty[:, :, :3]).all()
        agent.prefill(150)
        for more in (0, 3):
            for _ in range(more):
                agent.sample()
            got = agent.window_trend(8).numpy()
            assert got.shape == (len(agent.series), 9, 4) and got.dtype == np.float32
            s = 0
            for i, r in enumerate(agent.rings):
                rows, _ = agent.window_host(i)
                want = window_trend_reference(rows, r.head, 128, 8)
                np.testing.assert_array_equal(got[s:s + r.width].view(np.uint32), want.view(np.uint32))
                s += r.width
            assert got[:, :, 3].sum(axis=1).max() == 128
            h = agent.rings[0].head
            np.testing.assert_array_equal(agent.trend_age_rows(8), trend_age_rows(h, 128, 128, 8))
        with pytest.raises(ValueError):
            agent.window_trend(6)
        with pytest.raises(ValueError):
            agent.window_trend(256)
    finally:
        agent.close()


# ---- figure -----------------------------------------------------------------------------
_AGE = [30.0, 20.0, float("nan"), 10.0, 0.0]
_LO = [1.0, 2.0, float("nan"), 1.5, 0.5]
_HI = [4.0, 5.0, float("nan"), 4.5, 3.5]
_MEAN = [2.0, 3.0, float("nan"), 2.5, 1.5]


def test_create_trend_leaves_empty_slots_as_gaps():
    from rocmdash.viz.figures import create_trend

    fig = create_trend("Temperature", _AGE, np.array(_LO, np.float32), _HI, _MEAN, 100, 220)
    doc = json.loads(fig.to_json())  # strict JSON: no NaN
    assert [t["name"] for t in doc["data"]] == ["min", "max", "mean"]
    for t, y in zip(doc["data"], (_LO, _HI, _MEAN)):
        assert t["type"] == "scatter" and t["mode"] == "lines" and "connectgaps" not in t
        assert t["x"] == [-30.0, -20.0, None, -10.0, 0.0]
        assert t["y"] == [y[0], y[1], None, y[3], y[4]]
    assert doc["data"][1]["fill"] == "tonexty"  # the band: max down to min
    assert doc["layout"]["yaxis"]["range"] == [0, 100] and doc["layout"]["height"] == 220
    # a slot with an age but no valid sample is a gap too
    doc = json.loads(create_trend("t", [2.0, 1.0, 0.0], [1, float("nan"), 1], [2, float("nan"), 2], [1.5, float("nan"), 1.5]).to_json())
    assert doc["data"][2]["y"] == [1.5, None, 1.5] and doc["data"][2]["x"] == [-2.0, -1.0, 0.0]


@pytest.mark.parametrize("max_val", [100, 750.0])
def test_create_trend_json_matches_plotly(max_val):
    go = pytest.importorskip("plotly.graph_objects")
    from rocmdash.viz.figures import TREND_BAND, TREND_LINE, create_trend

    def none(v):
        return [None if x != x else x for x in v]

    x = [None if a != a else -a for a in _AGE]
    ref = go.Figure()
    ref.add_trace(go.Scatter(x=x, y=none(_LO), mode="lines", name="min", line=dict(width=0), hoverinfo="skip"))
    ref.add_trace(go.Scatter(x=x, y=none(_HI), mode="lines", name="max", line=dict(width=0), hoverinfo="skip",
                             fill="tonexty", fillcolor=TREND_BAND))
    ref.add_trace(go.Scatter(x=x, y=none(_MEAN), mode="lines", name="mean", line=dict(color=TREND_LINE, width=2)))
    ref.update_layout(title=dict(text="GPU 0: Power"), xaxis=dict(title=dict(text="seconds"), showgrid=True, gridcolor="lightgray"),
                      yaxis=dict(range=[0, max_val]), margin=dict(l=40, r=20, t=40, b=40), height=220, showlegend=False)
    ours = create_trend("GPU 0: Power", _AGE, _LO, _HI, _MEAN, max_val, 220)
    assert json.loads(ours.to_json()) == json.loads(ref.to_json())
    assert json.loads(ours.to_plotly().to_json()) == json.loads(ours.to_json())


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


def test_exporter_serves_trend_json_and_404_without(native, monkeypatch):
    """A synthetic source without a GPU: /trend is the documented JSON with null for NaN; off
    (the default) it is a 404; the trend never reaches /metrics."""
    import torch

    from rocmdash.prom.exporter import Exporter

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # agents on the CPU, wherever this runs
    monkeypatch.delenv("ROCMDASH_WINDOW_TREND", raising=False)
    src = _local_source(window_trend=8)
    exp = Exporter(src, hostname="n1")
    try:
        agent = src.agents[0]
        assert agent.dws is None
        agent.prefill(40)  # the window is not full: the oldest slots are empty
        exp.serve("127.0.0.1", 0)
        code, ctype, body = _get(exp.port, "/trend")
        assert code == 200 and ctype == "application/json"
        assert b"NaN" not in body
        doc = json.loads(body)
        assert doc["columns"] == 8 and doc["series"] == list(src.series) and list(doc["gpus"]) == [agent.info.gpu_id]
        assert len(doc["age_rows"]) == 9 and doc["age_rows"][-1] == 0 and doc["age_rows"][0] is None
        per = doc["gpus"][agent.info.gpu_id]
        assert set(per) == set(src.series)
        want = agent.window_trend(8).numpy()
        for s, metric in enumerate(src.series):
            m = per[metric]
            assert set(m) == {"min", "max", "mean", "count"}
            for i, k in enumerate(("min", "max", "mean", "count")):
                assert len(m[k]) == 9
                for v, w in zip(m[k], want[s, :, i]):
                    assert (v is None and math.isnan(w)) or v == float(w)
            assert m["count"][0] == 0 and m["min"][0] is None
        # (the samplers may have pushed a row or two before they were stopped)
        assert 40 <= sum(per[src.series[0]]["count"]) == agent.rings[0].head < 56
        metrics = _get(exp.port, "/metrics")[2].decode()
        assert "trend" not in metrics
    finally:
        exp.close()

    src = _local_source()
    exp = Exporter(src, hostname="n1")
    try:
        assert src.trend_columns is None
        exp.serve("127.0.0.1", 0)
        assert _get(exp.port, "/trend")[0] == 404
        assert _get(exp.port, "/metrics")[0] == 200
    finally:
        exp.close()


def test_metrics_are_byte_identical_with_the_trend_on_and_off(native):
    """The same snapshot with and without a trend renders the same /metrics text."""
    import copy

    from rocmdash.prom.exporter import SyntheticSource, render_trend
    from rocmdash.prom.exposition import render_snapshot

    snap, _ = SyntheticSource(2, seed=3).collect()
    snap.window_series = tuple(snap.columns[:3])
    snap.window = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    off = render_snapshot(snap, hostname="n1")
    assert render_trend(snap) is None
    on = copy.copy(snap)
    on.window_trend = np.full((2, 3, 9, 4), np.nan, np.float32)
    on.window_trend[:, :, 1:, :] = 2.5
    on.window_trend_age_rows = np.array([np.nan] + list(range(7, -1, -1)), np.float64)
    assert render_snapshot(on, hostname="n1") == off
    doc = json.loads(render_trend(on))
    assert doc["columns"] == 8 and doc["age_rows"][0] is None and doc["age_rows"][-1] == 0
    assert doc["gpus"][snap.gpu_ids[0]][snap.window_series[0]]["mean"] == [None] + [2.5] * 8


def test_exporter_option_from_the_environment(native, monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCMDASH_WINDOW_TREND", "16")
    src = _local_source()
    try:
        assert src.trend_columns == 16
        src.agents[0].prefill(70)
        snap, _ = src.collect()
        assert snap.window_trend.shape == (1, len(src.series), 17, 4) and snap.window_trend_age_rows.shape == (17,)
    finally:
        src.close()
    monkeypatch.setenv("ROCMDASH_WINDOW_TREND", "6")
    with pytest.raises(ValueError):
        _local_source()


# ---- page -------------------------------------------------------------------------------
def test_page_trend_figures_only_with_a_trend():
    from rocmdash.prom.exporter import SyntheticSource
    from rocmdash.ui.page import window_trend_figures
    from rocmdash.viz.panels import POWER, TEMP, UTIL

    snap, _ = SyntheticSource(2, seed=1).collect()
    assert window_trend_figures(snap, snap.gpu_ids) is None  # no trend: the page is as it was
    snap.window_series = (UTIL, TEMP, POWER, "amd_gpu_gfx_clock")
    snap.window_trend = np.full((2, 4, 9, 4), 1.0, np.float32)
    snap.window_trend[:, :, 0] = np.nan
    snap.window_trend_age_rows = np.array([np.nan] + list(range(70, -1, -10)), np.float64)
    figs = window_trend_figures(snap, [snap.gpu_ids[1]])
    assert [k for k, _ in figs] == [f"plot_trend_{m}_{snap.gpu_ids[1]}_" for m in ("gpu_util", "temp", "power")]
    doc = json.loads(figs[0][1].to_json())
    assert doc["data"][2]["y"] == [None] + [1.0] * 8 and doc["data"][2]["x"][0] is None and doc["data"][2]["x"][-1] == 0
