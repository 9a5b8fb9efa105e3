"""Window heatmap on the CPU (rocmdash.ops.window_heatmap states the semantics): the numpy
reference against a brute-force loop over rows, its two identities against the trend's and
the buckets' references, the argument rules, the kernels' compile-time resources, the agent
without a device, the figure, the exporter's /heatmap document and the page's charts."""

import json
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


# ---- reference --------------------------------------------------------------------------
def _brute(rows, head, W, P, bounds):
    """Row by row, in plain Python: the column of absolute row r is r // c, slot j is column
    (head - 1) // c - P + j, the bin is the number of bounds below the sample (fp32)."""
    n, S = rows.shape
    B = bounds.shape[1]
    c = W // P
    out = np.zeros((S, P + 1, B + 1), np.int64)
    for i in range(n):
        r = head - n + i
        j = r // c - ((head - 1) // c - P)
        assert 0 <= j <= P
        for s in range(S):
            x = np.float32(rows[i, s])
            if x != x:
                continue
            out[s, j, sum(1 for b in bounds[s] if np.float32(b) < x)] += 1
    return out


def _edge_rows(n, rng):
    """[n, 6]: ties on bounds, +-inf and NaN, signed zeroes, wide, a ramp, all NaN."""
    ties = rng.choice(np.array([-1.0, 0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 9.0], np.float32), n)
    inf = rng.normal(0, 3, n).astype(np.float32)
    inf[rng.random(n) < 0.1] = np.inf
    inf[rng.random(n) < 0.1] = -np.inf
    inf[rng.random(n) < 0.1] = np.nan
    zeroes = rng.choice(_exact.ZEROES, n)
    wide = _exact.family("wide_nan", rng, 0, n, n)
    ramp = np.arange(n, dtype=np.float32) / 4
    return np.stack([ties, inf, zeroes, wide, ramp, np.full(n, np.nan, np.float32)], axis=1)


_EVEN = np.arange(1, 9, dtype=np.float32)  # 1 .. 8
_UNEVEN = np.array([-1.0, 0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 1e30], np.float32)  # a bound of 0.0: -0.0 goes down with +0.0


@pytest.mark.parametrize("bounds", [_EVEN, _UNEVEN, np.array([0.0], np.float32)], ids=["even", "uneven", "one"])
@pytest.mark.parametrize("head_off", [0, 1, 2 * 64 + 37])
@pytest.mark.parametrize("n,W,P", [(1, 64, 8), (40, 64, 8), (64, 64, 64), (64, 64, 8), (100, 128, 16)])
def test_reference_against_a_per_row_loop(n, W, P, head_off, bounds):
    from rocmdash.ops.window_heatmap import window_heatmap_reference

    rng = np.random.default_rng(n + W + P + head_off)
    rows = _edge_rows(n, rng)
    head = n + head_off
    b = np.broadcast_to(bounds, (rows.shape[1], len(bounds)))
    got = window_heatmap_reference(rows, head, W, P, bounds)
    assert got.dtype == np.int32 and got.shape == (rows.shape[1], P + 1, len(bounds) + 1)
    np.testing.assert_array_equal(got, _brute(rows, head, W, P, b))
    assert got.sum() == np.count_nonzero(~np.isnan(rows))
    assert (got[5] == 0).all()  # the all-NaN series


def test_reference_bin_rule_at_the_edges():
    """Ties go down, -0.0 == +0.0, -inf in bin 0, +inf in bin B, NaN nowhere."""
    from rocmdash.ops.window_heatmap import window_heatmap_reference

    x = np.array([-np.inf, -0.0, 0.0, 1e-45, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.inf, np.nan], np.float32)
    got = window_heatmap_reference(x[:, None], 8, 8, 8, [0.0, 1.0])[0]
    assert got.shape == (9, 3)
    np.testing.assert_array_equal(got[0], [0, 0, 0])  # head 8, c = 1: slot 0 is column -1
    np.testing.assert_array_equal(got[1:], [[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1],
                                            [0, 0, 0]])
    assert (window_heatmap_reference(np.zeros((0, 3), np.float32), 0, 64, 8, [1.0, 2.0]) == 0).all()  # n == 0


@pytest.mark.parametrize("head_off", [0, 1, 3 * 256 - 1 - 200])
def test_reference_identities(head_off):
    """Per slot the bins sum to the trend's count; the slots summed and cumulated over the bins
    are the le-buckets of the same window."""
    from rocmdash.ops.window_buckets import bucket_ring_reference, window_buckets_reference
    from rocmdash.ops.window_heatmap import window_heatmap_reference
    from rocmdash.ops.window_trend import T_COUNT, window_trend_reference

    n, W, P = 200, 256, 16
    rng = np.random.default_rng(5 + head_off)
    rows = _exact.family_rows(rng, 0, n, W, width=len(_exact.FAMILIES), blips=(7,))
    head = n + head_off
    bounds = np.sort(rng.normal(50, 60, (rows.shape[1], 12)).astype(np.float32), axis=1)
    got = window_heatmap_reference(rows, head, W, P, bounds)
    with np.errstate(invalid="ignore", over="ignore"):
        trend = window_trend_reference(rows, head, W, P)
    np.testing.assert_array_equal(got.sum(axis=2), trend[:, :, T_COUNT])
    cum = np.cumsum(got.sum(axis=1), axis=1)
    np.testing.assert_array_equal(cum, window_buckets_reference(rows.T, bounds))
    ring = np.full((2 * W, rows.shape[1]), np.nan, np.float32)
    ring[np.arange(head - n, head) % (2 * W)] = rows
    np.testing.assert_array_equal(cum, bucket_ring_reference(ring, head, n, bounds))


# ---- arguments --------------------------------------------------------------------------
def test_parse_heatmap_and_argument_errors():
    from rocmdash.ops.window_heatmap import parse_heatmap, window_heatmap_reference

    assert parse_heatmap("64x16") == (64, 16)
    assert parse_heatmap(" 8X1 ") == (8, 1)
    assert parse_heatmap((1024, 63)) == (1024, 63)
    for bad in ("64", "64x", "x16", "64x16x2", "6x16", "4x16", "2048x16", "64x0", "64x64", "axb", "", (64,), 64, "64.0x16"):
        with pytest.raises(ValueError):
            parse_heatmap(bad)
    rows = np.zeros((64, 2), np.float32)
    ok = [1.0, 2.0]
    window_heatmap_reference(rows, 64, 64, 8, ok)
    for kw in (dict(columns=6), dict(columns=128), dict(head=63), dict(window=96), dict(bounds=[2.0, 1.0]),
               dict(bounds=[1.0, 1.0]), dict(bounds=[1.0, np.inf]), dict(bounds=[]), dict(bounds=np.arange(64.0)),
               dict(bounds=np.ones((3, 2))), dict(rows=np.zeros(64, np.float32))):
        a = dict(rows=rows, head=64, window=64, columns=8, bounds=ok)
        a.update(kw)
        with pytest.raises(ValueError):
            window_heatmap_reference(**a)
    with pytest.raises(ValueError):
        window_heatmap_reference(np.zeros((2, 1), np.float32), 2, 1 << 20, 8, ok)  # 2^17 rows per column


def test_constants_mirror_the_header():
    from rocmdash.ops import window_heatmap as wh

    text = open(os.path.join(ROOT, "csrc", "window_heatmap.h")).read()
    assert int(re.search(r"kHeatmapRingsPerLaunch = (\d+)", text).group(1)) == wh.RINGS_PER_LAUNCH
    trend = open(os.path.join(ROOT, "csrc", "window_trend.h")).read()
    assert int(re.search(r"kMaxTrendRowsPerColumn = (\d+)", trend).group(1)) == wh.MAX_COUNT


# ---- kernel resources -------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_heatmap_kernels_have_no_scratch_and_fit_lds(tmp_path):
    """The flags of test_trend_kernels_have_no_scratch_and_fit_lds; four workgroups stay
    resident per CU: LDS per block at most a quarter of the CU's."""
    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", "window_heatmap.hip"), "-o", str(tmp_path / "k.o"),
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
    assert len(kernels) >= 2, res.stderr[-2000:]  # a wave per slot, a workgroup per slot
    for k, r in kernels.items():
        assert r["ScratchSize [bytes/lane]"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] <= LDS_BYTES_PER_CU // 4, (k, r)


# ---- agent without a device -------------------------------------------------------------
def _cpu_agent(window=128):
    from rocmdash.config import SamplerConfig
    from rocmdash.runtime.agent import GpuAgent

    return GpuAgent(0, source="synthetic", counters="synthetic", cfg=SamplerConfig(window=window, ring_capacity=4 * window),
                    use_gpu=False)


def test_cpu_agent_window_heatmap(native):
    from rocmdash.ops.window_heatmap import window_heatmap_reference

    agent = _cpu_agent(128)
    try:
        assert agent.dws is None
        S = len(agent.series)
        empty = agent.window_heatmap(8).numpy()
        assert empty.shape == (S, 9, 17) and empty.dtype == np.int32 and (empty == 0).all()
        agent.prefill(150)
        default = agent.default_bucket_bounds(16)
        custom = np.sort(np.random.default_rng(1).uniform(0, 100, (S, 5)).astype(np.float32), axis=1)
        for more in (0, 3):
            for _ in range(more):
                agent.sample()
            for P, bounds, b in ((8, None, default), (64, None, default), (8, custom, custom)):
                got = agent.window_heatmap(P, bounds).numpy()
                assert got.shape == (S, P + 1, b.shape[1] + 1) and got.dtype == np.int32
                s = 0
                for i, r in enumerate(agent.rings):
                    rows, _ = agent.window_host(i)
                    want = window_heatmap_reference(rows, r.head, 128, P, b[s:s + r.width])
                    np.testing.assert_array_equal(got[s:s + r.width], want)
                    s += r.width
                assert got.sum(axis=(1, 2)).max() == 128
                np.testing.assert_array_equal(got.sum(axis=2), agent.window_trend(P).numpy()[:, :, 3])
        for bad in (dict(columns=6), dict(columns=256), dict(bounds=[2.0, 1.0]), dict(bounds=np.ones((S + 1, 2)))):
            with pytest.raises(ValueError):
                agent.window_heatmap(**bad)
    finally:
        agent.close()


# ---- figure -----------------------------------------------------------------------------
_AGE = [30.0, 20.0, float("nan"), 10.0, 0.0]
_LE = [25.0, 50.0, 75.0, 100.0]
_COUNTS = [[1, 2, 3, 4, 0], [0, 0, 10, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [5, 0, 0, 0, 5]]


def test_create_heatmap_leaves_empty_slots_as_gaps():
    from rocmdash.viz.figures import create_heatmap

    fig = create_heatmap("Temperature", _AGE, np.array(_LE, np.float32), np.array(_COUNTS, np.int32), 220)
    doc = json.loads(fig.to_json())  # strict JSON: no NaN
    assert len(doc["data"]) == 1
    t = doc["data"][0]
    assert t["type"] == "heatmap"
    assert t["x"] == [-30.0, -20.0, None, -10.0, 0.0]
    assert t["y"] == [25.0, 50.0, 75.0, 100.0, 125.0]  # the top bin: one bin above the axis maximum
    # z[bin][slot]; the slot without an age and the slot without a sample are null columns
    assert t["z"] == [[1, 0, None, None, 5], [2, 0, None, None, 0], [3, 10, None, None, 0], [4, 0, None, None, 0],
                      [0, 0, None, None, 5]]
    assert all(isinstance(v, int) for row in t["z"] for v in row if v is not None)
    y = doc["layout"]["yaxis"]
    assert y["tickvals"] == t["y"] and y["ticktext"] == ["25", "50", "75", "100", "> 100"]
    assert doc["layout"]["height"] == 220 and doc["layout"]["title"]["text"] == "Temperature"
    one = json.loads(create_heatmap("t", [1.0, 0.0], [4.0], [[1, 0], [0, 2]]).to_json())
    assert one["data"][0]["y"] == [4.0, 8.0] and one["data"][0]["z"] == [[1, 0], [0, 2]]
    many = json.loads(create_heatmap("t", [0.0], list(range(1, 64)), [[1] * 64]).to_json())
    assert len(many["layout"]["yaxis"]["tickvals"]) <= 17 and many["layout"]["yaxis"]["ticktext"][-1] == "> 63"


def test_create_heatmap_json_matches_plotly():
    go = pytest.importorskip("plotly.graph_objects")
    from rocmdash.viz.figures import create_heatmap

    x = [None if a != a else -a for a in _AGE]
    z = [[1, 0, None, None, 5], [2, 0, None, None, 0], [3, 10, None, None, 0], [4, 0, None, None, 0], [0, 0, None, None, 5]]
    ys = _LE + [125.0]
    ref = go.Figure()
    ref.add_trace(go.Heatmap(x=x, y=ys, z=z, zmin=0, hoverongaps=False, colorbar=dict(title=dict(text="samples"))))
    ref.update_layout(title=dict(text="GPU 0: Power"), xaxis=dict(title=dict(text="seconds")),
                      yaxis=dict(tickmode="array", tickvals=ys, ticktext=["25", "50", "75", "100", "> 100"]),
                      margin=dict(l=40, r=20, t=40, b=40), height=220, showlegend=False)
    ours = create_heatmap("GPU 0: Power", _AGE, _LE, _COUNTS, 220)
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


def _strict(body):
    def no_constant(name):
        raise AssertionError(f"{name} in a strict JSON document")

    return json.loads(body, parse_constant=no_constant)


def test_exporter_serves_heatmap_json_and_404_without(native, monkeypatch):
    """A synthetic source without a GPU: /heatmap is the documented strict JSON; off (the
    default) it is a 404 with a hint; the heatmap never reaches /metrics."""
    import torch

    from rocmdash.prom.exporter import Exporter

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # agents on the CPU, wherever this runs
    monkeypatch.delenv("ROCMDASH_WINDOW_HEATMAP", raising=False)
    src = _local_source(window_heatmap=(8, 5))
    exp = Exporter(src, hostname="n1")
    try:
        agent = src.agents[0]
        assert agent.dws is None and src.heatmap == (8, 5)
        agent.prefill(40)  # the window is not full: the oldest slots are empty
        exp.serve("127.0.0.1", 0)
        code, ctype, body = _get(exp.port, "/heatmap?x=1")
        assert code == 200 and ctype == "application/json"
        doc = _strict(body)
        assert set(doc) == {"columns", "buckets", "age_rows", "series", "gpus"}
        assert doc["columns"] == 8 and doc["buckets"] == 5 and doc["series"] == list(src.series)
        assert list(doc["gpus"]) == [agent.info.gpu_id]
        assert len(doc["age_rows"]) == 9 and doc["age_rows"][-1] == 0 and doc["age_rows"][0] is None
        per = doc["gpus"][agent.info.gpu_id]
        assert set(per) == set(src.series)
        want = agent.window_heatmap(8, src.heatmap_bounds).numpy()
        for s, metric in enumerate(src.series):
            m = per[metric]
            assert set(m) == {"le", "counts"}
            assert m["le"] == [float(v) for v in src.heatmap_bounds[s]] and len(m["le"]) == 5
            assert len(m["counts"]) == 9 and all(len(c) == 6 for c in m["counts"])
            assert all(isinstance(v, int) for c in m["counts"] for v in c)
            assert m["counts"] == want[s].tolist()
            assert m["counts"][0] == [0] * 6
        # (the samplers may have pushed a row or two before they were stopped)
        assert 40 <= sum(map(sum, per[src.series[0]]["counts"])) == agent.rings[0].head < 56
        metrics = _get(exp.port, "/metrics")[2].decode()
        assert "heatmap" not in metrics
    finally:
        exp.close()

    src = _local_source()
    exp = Exporter(src, hostname="n1")
    try:
        assert src.heatmap is None
        exp.serve("127.0.0.1", 0)
        code, _, body = _get(exp.port, "/heatmap")
        assert code == 404 and b"--window-heatmap" in body
        assert _get(exp.port, "/metrics")[0] == 200
    finally:
        exp.close()


def test_metrics_are_byte_identical_with_the_heatmap_on_and_off(native):
    """The same snapshot with and without a heatmap renders the same /metrics text."""
    import copy

    from rocmdash.prom.exporter import SyntheticSource, render_heatmap
    from rocmdash.prom.exposition import render_snapshot

    snap, _ = SyntheticSource(2, seed=3).collect()
    snap.window_series = tuple(snap.columns[:3])
    snap.window = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    off = render_snapshot(snap, hostname="n1")
    assert render_heatmap(snap) is None
    on = copy.copy(snap)
    on.window_heatmap = np.zeros((2, 3, 9, 5), np.int32)
    on.window_heatmap[:, :, 1:, 2] = 7
    on.window_heatmap_bounds = np.broadcast_to(np.array([1, 2, 3, 4], np.float32), (2, 3, 4))
    on.window_heatmap_age_rows = np.array([np.nan] + list(range(7, -1, -1)), np.float64)
    assert render_snapshot(on, hostname="n1") == off
    doc = _strict(render_heatmap(on))
    assert doc["columns"] == 8 and doc["buckets"] == 4 and doc["age_rows"][0] is None and doc["age_rows"][-1] == 0
    m = doc["gpus"][snap.gpu_ids[0]][snap.window_series[0]]
    assert m["le"] == [1.0, 2.0, 3.0, 4.0] and m["counts"] == [[0] * 5] + [[0, 0, 7, 0, 0]] * 8


def test_exporter_option_from_the_environment(native, monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCMDASH_WINDOW_HEATMAP", "16x4")
    src = _local_source()
    try:
        assert src.heatmap == (16, 4)
        src.agents[0].prefill(70)
        snap, _ = src.collect()
        S = len(src.series)
        assert snap.window_heatmap.shape == (1, S, 17, 5) and snap.window_heatmap.dtype == np.int32
        assert snap.window_heatmap_bounds.shape == (1, S, 4) and snap.window_heatmap_age_rows.shape == (17,)
    finally:
        src.close()
    for bad in ("6x4", "16x64", "128x4"):  # 128 columns for a window of 64 rows
        monkeypatch.setenv("ROCMDASH_WINDOW_HEATMAP", bad)
        with pytest.raises(ValueError):
            _local_source()


def test_exporter_command_line_rejects_a_bad_heatmap(capsys):
    from rocmdash.prom.exporter import main

    with pytest.raises(SystemExit):
        main(["--window-heatmap", "64x64"])
    assert "--window-heatmap" in capsys.readouterr().err


# ---- page -------------------------------------------------------------------------------
def test_page_heatmap_figures_only_with_a_heatmap():
    from rocmdash.prom.exporter import SyntheticSource
    from rocmdash.ui.page import window_heatmap_figures
    from rocmdash.viz.panels import POWER, TEMP, UTIL

    snap, _ = SyntheticSource(2, seed=1).collect()
    assert window_heatmap_figures(snap, snap.gpu_ids) is None  # no heatmap: the page is as it was
    snap.window_series = (UTIL, TEMP, POWER, "amd_gpu_gfx_clock")
    snap.window_heatmap = np.ones((2, 4, 9, 5), np.int32)
    snap.window_heatmap[:, :, 0] = 0
    snap.window_heatmap_bounds = np.broadcast_to(np.array([25, 50, 75, 100], np.float32), (2, 4, 4))
    snap.window_heatmap_age_rows = np.array([np.nan] + list(range(70, -1, -10)), np.float64)
    figs = window_heatmap_figures(snap, [snap.gpu_ids[1]])
    assert [k for k, _ in figs] == [f"plot_heatmap_{m}_{snap.gpu_ids[1]}_" for m in ("gpu_util", "temp", "power")]
    doc = json.loads(figs[0][1].to_json())
    t = doc["data"][0]
    assert t["type"] == "heatmap" and t["x"][0] is None and t["x"][-1] == 0
    assert t["z"] == [[None] + [1] * 8] * 5
