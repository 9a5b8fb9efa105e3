"""Window distributions as cumulative le-buckets (rocmdash.ops.window_buckets and the layers
above it), CPU side: the exact reference's semantics, the default bounds, the exposition
round trip, PromQL's histogram_quantile, the agent's CPU path, the world-1 node sum, and
the kernel's compile-time resources."""

import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAN, INF = float("nan"), float("inf")


# ---- reference semantics --------------------------------------------------------------
def test_reference_ties_zeros_infinities_nan():
    from rocmdash.ops.window_buckets import window_buckets_reference

    x = np.array([
        [1.0, 2.0, 2.0, 3.0, 2.0, 5.0],        # ties on a bound count as <=
        [-0.0, 0.0, -1.0, 1.0, 0.0, -0.0],     # -0.0 == +0.0
        [-INF, INF, 0.5, NAN, INF, -INF],      # -inf in every bucket, +inf only in +Inf, NaN in none
        [NAN] * 6,                             # all NaN
        [1e-45, -1e-45, 1e-40, -1e-40, 0.0, 3e-45],  # denormals are values, not zeros
    ], np.float32)
    bounds = np.array([
        [2.0, 4.0],
        [-0.0, 0.5],
        [0.0, 1.0],
        [0.0, 1.0],
        [0.0, 1e-45],
    ], np.float32)
    got = window_buckets_reference(x, bounds)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, [
        [4, 5, 6],
        [5, 5, 6],
        [2, 3, 5],
        [0, 0, 0],
        [3, 4, 6],
    ])
    # one row of bounds serves every series; +0.0 as a bound counts -0.0 samples
    np.testing.assert_array_equal(window_buckets_reference(x[:2], [0.0, 2.0]), [[0, 4, 6], [5, 6, 6]])


def test_reference_empty_window_and_bad_bounds():
    from rocmdash.ops.window_buckets import window_buckets_reference

    np.testing.assert_array_equal(window_buckets_reference(np.zeros((2, 0), np.float32), [1.0, 2.0]), np.zeros((2, 3)))
    x = np.zeros((1, 4), np.float32)
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [1.0, INF], [NAN], list(range(64)), [[1.0], [2.0]]):
        with pytest.raises(ValueError):
            window_buckets_reference(x, bad)
    assert window_buckets_reference(x, list(range(63))).shape == (1, 64)


def test_default_bounds_ascending_finite_for_every_series():
    from rocmdash.models.schema import METRIC_SPECS, series_names
    from rocmdash.ops.window_buckets import default_bounds

    names = series_names()
    for buckets in (1, 16, 63):
        b = default_bounds(names, buckets=buckets)
        assert b.shape == (len(names), buckets) and b.dtype == np.float32
        assert np.isfinite(b).all() and (b > 0).all()
        assert (np.diff(b, axis=1) > 0).all()
    b = default_bounds(names, power_limit_w=1400.0, total_vram_mb=294912.0)
    for i, n in enumerate(names):
        spec = METRIC_SPECS[n]
        if spec.axis_max:
            assert b[i, -1] == np.float32(spec.axis_max), n
    assert b[names.index("amd_gpu_average_package_power"), -1] == 1400.0
    assert b[names.index("amd_gpu_used_vram"), -1] == b[names.index("amd_gpu_total_vram"), -1] == 294912.0
    # no cap known: the page's power axis for the part number (300 W for an unknown one)
    assert default_bounds(names)[names.index("amd_gpu_average_package_power"), -1] == 300.0
    assert default_bounds(names, card_model="102-G36236-0C")[names.index("amd_gpu_average_package_power"), -1] == 1400.0
    with pytest.raises(ValueError):
        default_bounds(names, buckets=64)


def test_share_above():
    from rocmdash.ops.window_buckets import share_above

    counts, bounds = [10, 40, 90, 100], [25.0, 50.0, 75.0]
    assert share_above(counts, bounds, 50.0) == 0.6
    assert share_above(counts, bounds, 74.9) == 0.6  # the largest bound <= threshold
    assert share_above(counts, bounds, 1000.0) == pytest.approx(0.1)
    assert math.isnan(share_above(counts, bounds, 10.0)) and math.isnan(share_above([0, 0, 0, 0], bounds, 50.0))


# ---- exposition -----------------------------------------------------------------------
SERIES = ("amd_gpu_average_package_power", "amd_gpu_junction_temperature")  # in snapshot_io.VALUE_SERIES order


def _snap(buckets=False, rng=None):
    from rocmdash.models.schema import NUM_STATS
    from rocmdash.ops.window_buckets import window_buckets_reference
    from rocmdash.viz.panels import NodeSnapshot

    snap = NodeSnapshot(gpu_ids=["0", "1"], card_models=["102-G36236-0C"] * 2, columns=SERIES,
                        values=[[500.0, 70.0], [900.0, 80.0]], window=np.ones((2, 2, NUM_STATS)), window_series=SERIES)
    if buckets:
        bounds = np.array([[350.0, 700.0, 1050.0, 1400.0], [27.5, 55.0, 82.5, 110.0]], np.float32)
        x = rng.normal([[[800.0], [75.0]]], [[[300.0], [15.0]]], (2, 2, 256)).astype(np.float32)
        x[0, 0, :9] = np.nan
        per = np.stack([window_buckets_reference(x[g], bounds) for g in range(2)]).astype(np.float32)
        snap.window_buckets, snap.window_bucket_bounds, snap.node_window_buckets = per, bounds, per.sum(axis=0)
        return snap, x
    return snap


def test_render_snapshot_buckets_round_trip():
    from rocmdash.prom.exposition import parse_text, render_snapshot
    from rocmdash.prom.snapshot_io import snapshot_from_series

    snap, x = _snap(True, np.random.default_rng(5))
    text = render_snapshot(snap, hostname="n1")
    for fam in ("rocmdash_window_bucket", "rocmdash_node_window_bucket"):
        assert f"# TYPE {fam} gauge" in text
        help_ = next(line for line in text.split("\n") if line.startswith(f"# HELP {fam} "))
        assert "goes down as well as up" in help_ and "no counter histogram" in help_
    samples = parse_text(text)
    per = [s for s in samples if s.name == "rocmdash_window_bucket"]
    node = [s for s in samples if s.name == "rocmdash_node_window_bucket"]
    assert len(per) == 2 * 2 * 5 and len(node) == 2 * 5
    assert all(set(s.label_dict()) == {"gpu_id", "card_model", "hostname", "metric", "le"} for s in per)
    assert all(set(s.label_dict()) == {"hostname", "metric", "le"} for s in node)
    for g in range(2):
        for si, series in enumerate(SERIES):
            rows = [s for s in per if s.label_dict()["gpu_id"] == str(g) and s.label_dict()["metric"] == series]
            les = [s.label_dict()["le"] for s in rows]
            assert les == [repr(float(b)) for b in snap.window_bucket_bounds[si]] + ["+Inf"]  # in order, +Inf last
            counts = [s.value for s in rows]
            assert counts == sorted(counts) and counts == list(snap.window_buckets[g, si])  # cumulative
            assert counts[-1] == np.count_nonzero(~np.isnan(x[g, si]))  # +Inf = the valid count
    got = {(s.label_dict()["metric"], s.label_dict()["le"]): s.value for s in node}
    assert got[(SERIES[0], "+Inf")] == 2 * 256 - 9 and got[(SERIES[0], "1400.0")] == snap.node_window_buckets[0, 3]
    # ... and back into a snapshot (the page's native / extended Prometheus modes)
    items = [(dict(s.label_dict(), __name__=s.name), s.value) for s in samples]
    back = snapshot_from_series(items, require_vram=False)
    np.testing.assert_array_equal(back.window_bucket_bounds, snap.window_bucket_bounds)
    np.testing.assert_array_equal(back.window_buckets, snap.window_buckets)
    np.testing.assert_array_equal(back.node_window_buckets, snap.node_window_buckets)


def test_render_snapshot_unchanged_without_buckets():
    from rocmdash.prom.exposition import render_snapshot

    never = _snap()
    text = render_snapshot(never, hostname="n1")
    assert "_bucket" not in text
    had, _ = _snap(True, np.random.default_rng(5))
    had.timestamp = never.timestamp
    had.window_buckets = had.window_bucket_bounds = had.node_window_buckets = None
    assert render_snapshot(had, hostname="n1") == text


def test_page_bucket_table():
    from rocmdash.ui.page import window_bucket_table

    assert window_bucket_table(_snap()) is None
    snap, x = _snap(True, np.random.default_rng(5))
    table = window_bucket_table(snap)
    assert list(table) == list(SERIES)
    v = x[:, 1][~np.isnan(x[:, 1])]
    row = table[SERIES[1]]
    assert row["axis"] == 110.0 and row["samples"] == v.size
    assert row["> 50% of axis (%)"] == round(100.0 * np.count_nonzero(v > np.float32(55.0)) / v.size, 2)
    assert row["> 75% of axis (%)"] == round(100.0 * np.count_nonzero(v > np.float32(82.5)) / v.size, 2)
    # 90 % of the axis is no bound: the share above the largest bound below it (82.5)
    assert row["> 90% of axis (%)"] == row["> 75% of axis (%)"]


# ---- histogram_quantile ---------------------------------------------------------------
def test_bucket_quantile_by_hand():
    from rocmdash.prom.promql import bucket_quantile

    b = [(10.0, 10.0), (20.0, 30.0), (40.0, 40.0), (INF, 50.0)]
    assert bucket_quantile(0.5, b) == 10.0 + 10.0 * (25.0 - 10.0) / 20.0  # rank 25 in (10, 20]: 20 samples
    assert bucket_quantile(0.1, b) == 0.0 + 10.0 * 5.0 / 10.0  # first bucket: lower edge 0
    assert bucket_quantile(0.2, b) == 10.0  # rank 10 = the first bucket's count: its bound
    assert bucket_quantile(0.7, b) == 20.0 + 20.0 * 5.0 / 10.0
    assert bucket_quantile(0.9, b) == 40.0  # in +Inf: the highest finite bound
    assert bucket_quantile(1.0, b) == 40.0
    assert bucket_quantile(0.0, b) == 0.0
    assert bucket_quantile(0.5, list(reversed(b))) == 17.5  # sorted by le
    assert bucket_quantile(0.5, [(-5.0, 10.0), (5.0, 10.0), (INF, 10.0)]) == -5.0  # first bound <= 0: itself
    assert math.isnan(bucket_quantile(0.5, [(10.0, 0.0), (INF, 0.0)]))  # no samples
    assert math.isnan(bucket_quantile(0.5, [(10.0, 5.0), (20.0, 9.0)]))  # no +Inf bucket
    assert math.isnan(bucket_quantile(0.5, [(INF, 9.0)])) and math.isnan(bucket_quantile(0.5, []))
    assert math.isnan(bucket_quantile(NAN, b)) and bucket_quantile(-0.1, b) == -INF and bucket_quantile(1.1, b) == INF


def test_histogram_quantile_parse_and_grouping():
    from rocmdash.prom.promql import Aggregate, HistogramQuantile, PromQLError, Selector, histogram_quantile, parse

    e = parse('histogram_quantile(0.99, sum by (le) (rocmdash_window_bucket{metric="amd_gpu_junction_temperature"}))')
    assert isinstance(e, HistogramQuantile) and e.phi == 0.99
    assert isinstance(e.inner, Aggregate) and e.inner.op == "sum" and e.inner.by == ("le",)
    e = parse("histogram_quantile(.5,rocmdash_window_bucket)")
    assert isinstance(e.inner, Selector) and e.phi == 0.5
    assert parse("histogram_quantile(1e-1, sum(x) by (le, metric))").inner.by == ("le", "metric")
    for bad in ("histogram_quantile(x, y)", "histogram_quantile(0.5 y)", "histogram_quantile(0.5, y", "histogram_quantile(0.5, y) z"):
        with pytest.raises(PromQLError):
            parse(bad)
    rows = [({"__name__": "b", "gpu_id": g, "le": le}, c) for g, cs in (("0", (1, 4)), ("1", (3, 4)))
            for le, c in zip(("1.0", "+Inf"), cs)] + [({"__name__": "b", "gpu_id": "2"}, 7.0)]  # no le: ignored
    got = {labels["gpu_id"]: v for labels, v in histogram_quantile(0.5, rows)}
    assert got == {"0": 1.0, "1": 1.0 * 2.0 / 3.0}
    assert all("le" not in labels and "__name__" not in labels for labels, _ in histogram_quantile(0.5, rows))


def _mini_with(snap):
    from rocmdash.prom.exposition import parse_text, render_snapshot
    from rocmdash.prom.mini import MiniPrometheus

    prom = MiniPrometheus()
    prom.db.add_many([(dict(s.label_dict(), __name__=s.name, instance="n1:9400"), s.value)
                      for s in parse_text(render_snapshot(snap))])
    return prom


def _value(data):
    assert data["resultType"] == "vector" and len(data["result"]) == 1, data
    return data["result"][0]["metric"], float(data["result"][0]["value"][1])


def test_histogram_quantile_through_mini_prometheus_across_gpus():
    """sum by (le) of two GPUs' buckets, then the quantile: by hand, and through the HTTP API's JSON."""
    import json

    from rocmdash.prom.promql import bucket_quantile

    snap, _ = _snap(True, np.random.default_rng(11))
    prom = _mini_with(snap)
    q = 'histogram_quantile(0.9, sum by (le) (rocmdash_window_bucket{metric="amd_gpu_average_package_power"}))'
    labels, v = _value(prom.query(q))
    assert labels == {}
    summed = (snap.window_buckets[0, 0] + snap.window_buckets[1, 0]).tolist()
    want = bucket_quantile(0.9, list(zip(list(snap.window_bucket_bounds[0]) + [INF], summed)))
    assert v == want and 350.0 < v <= 1400.0
    # the node family carries the same sum; a plain selector groups by every label but le
    labels, v2 = _value(prom.query('histogram_quantile(0.9, rocmdash_node_window_bucket{metric="amd_gpu_average_package_power"})'))
    assert v2 == want and labels == {"metric": "amd_gpu_average_package_power", "instance": "n1:9400"}
    per_gpu = prom.query('histogram_quantile(0.9, rocmdash_window_bucket{metric="amd_gpu_average_package_power"})')
    assert sorted(r["metric"]["gpu_id"] for r in per_gpu["result"]) == ["0", "1"]
    body = json.loads(prom.query_json(q))
    assert body["status"] == "success" and float(body["data"]["result"][0]["value"][1]) == want
    assert prom.query('histogram_quantile(0.9, sum by (le) (rocmdash_window_bucket{metric="nope"}))')["result"] == []


def test_histogram_quantile_lies_in_the_exact_percentiles_bucket():
    """A window of 4096 seeded samples in 16 buckets: the rank histogram_quantile interpolates
    at, q * n, lies in the same cumulative-count step as numpy's 'linear' percentile position
    q * (n - 1) unless that position falls between two buckets - so the estimate lies in the
    bucket of the order statistics around the exact percentile: derived, nothing measured."""
    from rocmdash.ops.window_buckets import default_bounds, window_buckets_reference
    from rocmdash.viz.panels import NodeSnapshot

    series = ("amd_gpu_junction_temperature",)
    rng = np.random.default_rng(4096)
    x = np.clip(rng.normal(78.0, 9.0, (1, 4096)), 0, None).astype(np.float32)
    bounds = default_bounds(series)
    counts = window_buckets_reference(x, bounds).astype(np.float32)
    snap = NodeSnapshot(gpu_ids=["0"], card_models=[""], columns=series, values=[[x[0, -1]]],
                        window=np.ones((1, 1, 8)), window_series=series, window_buckets=counts[None],
                        window_bucket_bounds=bounds, node_window_buckets=counts)
    prom = _mini_with(snap)
    edges = np.concatenate([[0.0], bounds[0].astype(np.float64)])
    xs = np.sort(x[0]).astype(np.float64)
    for q in (0.5, 0.9, 0.99):
        _, v = _value(prom.query(f"histogram_quantile({q}, sum by (le) (rocmdash_node_window_bucket))"))
        pos = q * (len(xs) - 1)
        lo_x, hi_x = xs[int(math.floor(pos))], xs[int(math.ceil(pos))]  # np.percentile lies in [lo_x, hi_x]
        exact = float(np.percentile(xs, 100 * q))
        assert lo_x <= exact <= hi_x
        # the buckets (lower edge exclusive, upper inclusive) of the two order statistics
        b_lo = int(np.searchsorted(edges, lo_x, side="left")) - 1
        b_hi = int(np.searchsorted(edges, hi_x, side="left")) - 1
        assert 0 <= b_lo <= b_hi < len(bounds[0])
        assert edges[b_lo] <= v <= edges[b_hi + 1], (q, v, exact, edges[b_lo], edges[b_hi + 1])
        if b_lo == b_hi:  # the usual case: the one bucket that holds the exact value
            assert edges[b_lo] < exact <= edges[b_lo + 1]


# ---- agent, node sum ------------------------------------------------------------------
def _cpu_agent(window=128):
    from rocmdash.config import SamplerConfig
    from rocmdash.runtime.agent import GpuAgent

    return GpuAgent(0, source="synthetic", counters="synthetic", cfg=SamplerConfig(window=window, ring_capacity=4 * window),
                    use_gpu=False)


def test_cpu_agent_window_buckets(native):
    from rocmdash.models.schema import CTR_FIELDS, SMI_FIELDS
    from rocmdash.ops.window_buckets import window_buckets_reference

    agent = _cpu_agent()
    try:
        agent.prefill(200)
        st = agent.refresh().numpy()
        got = agent.window_buckets().numpy()
        bounds = agent.default_bucket_bounds()
        S = len(SMI_FIELDS) + len(CTR_FIELDS)
        assert got.shape == (S, 17) and got.dtype == np.float32 and bounds.shape == (S, 16)
        want = np.concatenate([window_buckets_reference(agent.window_host(i)[0].T, b) for i, b in
                               enumerate((bounds[: len(SMI_FIELDS)], bounds[len(SMI_FIELDS):]))])
        np.testing.assert_array_equal(got.astype(np.int64), want)
        np.testing.assert_array_equal(got[:, -1], st[:, 7])  # +Inf bucket = the stats' count
        assert got[:, -1].max() == 128
        mine = np.array([10.0, 50.0, 90.0], np.float32)
        np.testing.assert_array_equal(agent.window_buckets(mine).numpy()[: len(SMI_FIELDS)].astype(np.int64),
                                      window_buckets_reference(agent.window_host(0)[0].T, mine))
        with pytest.raises(ValueError):
            agent.window_buckets(np.array([2.0, 1.0], np.float32))
    finally:
        agent.close()


def test_cpu_agent_window_buckets_before_any_sample(native):
    agent = _cpu_agent()
    try:
        np.testing.assert_array_equal(agent.window_buckets().numpy(), np.zeros((len(agent.series), 17), np.float32))
    finally:
        agent.close()


def test_node_buckets_world1_and_mismatched_bounds(native):
    from rocmdash.parallel.node import NodeAggregator
    from rocmdash.parallel.node_buckets import NodeBuckets

    agent = _cpu_agent(64)
    try:
        agent.prefill(70)
        agent.refresh()
        agg = NodeAggregator()
        nb = NodeBuckets(agent, agg, agent.default_bucket_bounds(8))
        per_gpu, node = nb.refresh()
        S = len(agent.series)
        assert per_gpu.shape == (1, S, 9) and node.shape == (S, 9)
        np.testing.assert_array_equal(per_gpu[0], agent.window_buckets(nb.bounds).numpy())
        np.testing.assert_array_equal(node, per_gpu.sum(axis=0))
        assert node[:, -1].max() == 64

        class TwoRanks:  # a second rank that came up with other bounds
            rank, world_size = 0, 2

            def all_gather_object(self, obj):
                return [obj, (np.frombuffer(obj, np.float32) * 2).tobytes()]

        with pytest.raises(ValueError, match="differ between ranks"):
            NodeBuckets(agent, TwoRanks(), agent.default_bucket_bounds(8))
        with pytest.raises(ValueError):
            NodeBuckets(agent, agg, np.zeros((3, 4), np.float32))  # not this agent's series
    finally:
        agent.close()


def test_serve_refuses_buckets_with_a_long_window(monkeypatch, capsys):
    from rocmdash import serve

    monkeypatch.setenv("ROCMDASH_WINDOW", str(1 << 16))
    monkeypatch.setenv("ROCMDASH_RING_CAPACITY", str(1 << 16))
    with pytest.raises(SystemExit) as e:
        serve.main(["--cpu", "--window-buckets", "16"])
    assert e.value.code == 2 and "32768" in capsys.readouterr().err
    monkeypatch.delenv("ROCMDASH_WINDOW")
    with pytest.raises(SystemExit):
        serve.main(["--cpu", "--window-buckets", "64"])


# ---- the kernel's resources -----------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_window_buckets_kernels_have_no_scratch(tmp_path):
    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", "window_buckets.hip"), "-o", str(tmp_path / "k.o"),
         "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600,
    )
    assert res.returncode == 0, res.stderr[-3000:]
    kernels = {}
    name = None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs): (\d+)", line)
        if m and name is not None:
            kernels[name][m.group(1)] = int(m.group(2))
    assert len(kernels) == 2, res.stderr[-2000:]
    assert any("export_buckets_kernel" in k for k in kernels) and any("bucket_blocks_kernel" in k for k in kernels)
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", -1) == 0, (k, r)
        assert r.get("LDS Size [bytes/block]", -1) == 0, (k, r)  # registers only: no static LDS either


def test_service_refresh_fills_the_snapshot_and_metrics(native):
    """One service refresh (world 1, CPU) with buckets on: the snapshot carries the three
    fields and the exporter's text both families; without, the snapshot has none."""
    from rocmdash import serve
    from rocmdash.parallel.node import NodeAggregator
    from rocmdash.parallel.node_buckets import NodeBuckets
    from rocmdash.prom.exporter import Exporter
    from rocmdash.prom.exposition import parse_text
    from rocmdash.runtime.pipeline import NodePipeline

    agent = _cpu_agent(64)
    try:
        agent.prefill(70)
        agg = NodeAggregator()
        pipe = NodePipeline(agent, agg, device_timing=True, health=True)
        latest = serve._Latest()
        serve.refresh_node(pipe, agg, None, latest)
        snap, _ = latest.collect()
        assert snap.window_buckets is None and snap.window_bucket_bounds is None and snap.node_window_buckets is None
        nbk = NodeBuckets(agent, agg, agent.default_bucket_bounds(8))
        serve.refresh_node(pipe, agg, None, latest, nbk=nbk)
        snap, _ = latest.collect()
        S = len(agent.series)
        assert snap.window_buckets.shape == (1, S, 9) and snap.node_window_buckets.shape == (S, 9)
        np.testing.assert_array_equal(snap.window_bucket_bounds, nbk.bounds)
        np.testing.assert_array_equal(snap.node_window_buckets[:, -1], snap.window[0, :, 7])
        names = {s.name for s in parse_text(Exporter(latest, hostname="n1").render())}
        assert {"rocmdash_window_bucket", "rocmdash_node_window_bucket"} <= names
        pipe.close()
    finally:
        agent.close()
