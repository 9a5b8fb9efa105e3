"""Window joint histogram on the CPU (rocmdash.ops.window_joint states the semantics): the numpy
reference against a per-row loop, its three identities against the buckets' reference, the
argument rules, the kernel's compile-time resources, the host planning header under sanitizers,
the agent without a device, the figure, the exporter's /joint document and the page's charts."""

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
CAPTURE = os.path.join(ROOT, "tests", "fixtures", "mi355x_capture.npz")
LDS_BYTES_PER_WORKGROUP = 64 * 1024


# ---- reference --------------------------------------------------------------------------
def _brute(rows, pairs, bounds):
    """Row by row, in plain Python: the bin is the number of bounds below the sample (fp32); a row
    counts for a pair when neither sample is NaN."""
    B = bounds.shape[1]
    out = np.zeros((len(pairs), B + 1, B + 1), np.int64)
    for row in rows:
        for k, (a, b) in enumerate(pairs):
            x, y = np.float32(row[a]), np.float32(row[b])
            if x != x or y != y:
                continue
            i = sum(1 for v in bounds[a] if np.float32(v) < x)
            j = sum(1 for v in bounds[b] if np.float32(v) < y)
            out[k, i, j] += 1
    return out


def _edge_rows(n, rng):
    """[n, 6]: ties on bounds, +-inf and NaN, signed zeroes, wide with NaNs, a ramp, all NaN."""
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
_PAIRS = [(0, 1), (1, 0), (1, 3), (3, 1), (2, 0), (4, 2), (0, 5), (3, 4)]  # NaNs in one series, in both, in neither


@pytest.mark.parametrize("bounds", [_EVEN, _UNEVEN, np.array([0.0], np.float32)], ids=["even", "uneven", "one"])
@pytest.mark.parametrize("n", [1, 40, 257])
def test_reference_against_a_per_row_loop(n, bounds):
    from rocmdash.ops.window_joint import window_joint_reference

    rng = np.random.default_rng(n + len(bounds))
    rows = _edge_rows(n, rng)
    b = np.broadcast_to(bounds, (rows.shape[1], len(bounds)))
    got = window_joint_reference(rows, _PAIRS, bounds)
    assert got.dtype == np.int32 and got.shape == (len(_PAIRS), len(bounds) + 1, len(bounds) + 1)
    np.testing.assert_array_equal(got, _brute(rows, _PAIRS, b))
    assert (got[6] == 0).all()  # a pair with the all-NaN series
    for k, (a, c) in enumerate(_PAIRS):
        assert got[k].sum() == np.count_nonzero(~np.isnan(rows[:, a]) & ~np.isnan(rows[:, c]))


def test_reference_bin_rule_at_the_edges():
    """Ties go down, -0.0 == +0.0, -inf in bin 0, +inf in bin B, a NaN in either series drops the row."""
    from rocmdash.ops.window_joint import window_joint_reference

    x = np.array([-np.inf, -0.0, 0.0, 1e-45, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.inf, np.nan, 0.5], np.float32)
    y = np.array([0.5, 0.5, np.inf, -np.inf, 1.0, 0.0, np.nan, 0.5, np.nan], np.float32)
    got = window_joint_reference(np.stack([x, y], axis=1), [(0, 1)], [0.0, 1.0])[0]
    #             y: bin 0  1  2
    np.testing.assert_array_equal(got, [[0, 2, 1],   # x in bin 0: -inf, -0.0 (y 0.5), +0.0 (y +inf)
                                        [1, 1, 0],   # x in bin 1: 1e-45 (y -inf), 1.0 (y 1.0: tie down)
                                        [1, 0, 0]])  # x in bin 2: just above 1 (y 0.0)
    assert (window_joint_reference(np.zeros((0, 3), np.float32), [(0, 2)], [1.0, 2.0]) == 0).all()  # n == 0


def test_reference_identities():
    """A pair's cells sum to the rows valid in both; without NaNs the row and column sums are the
    de-cumulated le-buckets of a and of b; (b, a) is the transpose of (a, b)."""
    from rocmdash.ops.window_buckets import window_buckets_reference
    from rocmdash.ops.window_joint import window_joint_reference

    n = 300
    rng = np.random.default_rng(5)
    rows = _exact.family_rows(rng, 0, n, n, width=len(_exact.FAMILIES), blips=(7,))
    S = rows.shape[1]
    bounds = np.sort(rng.normal(50, 60, (S, 12)).astype(np.float32), axis=1)
    clean = [s for s in range(S) if not np.isnan(rows[:, s]).any()]
    dirty = [s for s in range(S) if np.isnan(rows[:, s]).any() and not np.isnan(rows[:, s]).all()]
    assert len(clean) >= 4 and len(dirty) >= 2
    pairs = [(clean[0], clean[1]), (clean[1], clean[0]), (clean[2], clean[3]), (dirty[0], dirty[1]), (dirty[1], dirty[0]),
             (clean[0], dirty[0])]
    got = window_joint_reference(rows, pairs, bounds)
    cum = window_buckets_reference(rows.T, bounds)  # [S, B + 1]: cumulative, then the valid count
    marg = np.diff(np.concatenate([np.zeros((S, 1), np.int64), cum], axis=1), axis=1)
    for k, (a, b) in enumerate(pairs):
        both = ~np.isnan(rows[:, a]) & ~np.isnan(rows[:, b])
        assert got[k].sum() == np.count_nonzero(both)
        if a in clean and b in clean:
            np.testing.assert_array_equal(got[k].sum(axis=1), marg[a])
            np.testing.assert_array_equal(got[k].sum(axis=0), marg[b])
    assert got[3].sum() < n
    np.testing.assert_array_equal(got[1], got[0].T)
    np.testing.assert_array_equal(got[4], got[3].T)
    # the result does not depend on how the window is chunked
    np.testing.assert_array_equal(sum(window_joint_reference(rows[i:i + 77], pairs, bounds) for i in range(0, n, 77)), got)


# ---- arguments --------------------------------------------------------------------------
def test_check_pairs_accepts_and_refuses():
    from rocmdash.ops.window_joint import MAX_PAIRS, check_pairs

    assert MAX_PAIRS == 8
    assert check_pairs([(0, 1)], 2) == [(0, 1)]
    assert check_pairs(np.array([[0, 10], [11, 15], [15, 11]]), (11, 5)) == [(0, 10), (11, 15), (15, 11)]
    assert check_pairs([(0, 1)] * 8, [2]) == [(0, 1)] * 8  # a pair may be named twice
    with pytest.raises(ValueError, match="spans rings 0 and 1.*no common row number"):
        check_pairs([(10, 11)], (11, 5))
    with pytest.raises(ValueError, match="spans rings"):
        check_pairs([(0, 1), (12, 2)], (11, 5))
    with pytest.raises(ValueError, match="two different series"):
        check_pairs([(3, 3)], (11, 5))
    with pytest.raises(ValueError, match="1 to 8 pairs, got 9"):
        check_pairs([(0, 1 + i) for i in range(9)], (11, 5))
    for bad in ([], [(0, 16)], [(-1, 0)], [(0, 1, 2)], [0, 1], None, [("a", "b")]):
        with pytest.raises(ValueError):
            check_pairs(bad, (11, 5))


def test_parse_joint_accepts_and_refuses():
    from rocmdash.models.schema import CTR_FIELDS, SMI_FIELDS
    from rocmdash.ops.window_joint import DEFAULT_BUCKETS, DEFAULT_PAIRS, MAX_JOINT_BUCKETS, parse_joint

    series, widths = SMI_FIELDS + CTR_FIELDS, (len(SMI_FIELDS), len(CTR_FIELDS))
    ix = series.index
    assert DEFAULT_BUCKETS == 16 and MAX_JOINT_BUCKETS == 31
    assert DEFAULT_PAIRS == (("mfma_utilization", "hbm_read_bandwidth"), ("mfma_utilization", "hbm_write_bandwidth"),
                             ("gfx_activity", "average_package_power"), ("average_package_power", "junction_temperature"))
    want = [(ix("amd_gpu_" + a), ix("amd_gpu_" + b)) for a, b in DEFAULT_PAIRS]
    assert parse_joint("default", series, widths) == (want, 16)
    assert parse_joint(" default/31 ", series, widths) == (want, 31)
    assert parse_joint("default", SMI_FIELDS) == (want[2:], 16)  # no counter ring: its pairs are left out
    assert parse_joint("gfx_activity:amd_gpu_xgmi_write_bandwidth, amd_gpu_mfma_utilization:gfx_busy/8", series, widths) == (
        [(ix("amd_gpu_gfx_activity"), ix("amd_gpu_xgmi_write_bandwidth")), (ix("amd_gpu_mfma_utilization"), ix("amd_gpu_gfx_busy"))], 8)
    with pytest.raises(ValueError, match="spans rings.*no common row number"):
        parse_joint("gfx_activity:mfma_utilization", series, widths)
    with pytest.raises(ValueError, match="two different series"):
        parse_joint("gfx_activity:gfx_activity", series, widths)
    with pytest.raises(ValueError, match="1 to 8 pairs, got 9"):
        parse_joint(",".join(["gfx_activity:average_package_power"] * 9), series, widths)
    with pytest.raises(ValueError, match="1 to 31 buckets.*got 32"):
        parse_joint("default/32", series, widths)
    with pytest.raises(ValueError, match="unknown metric 'warp_speed'"):
        parse_joint("gfx_activity:warp_speed", series, widths)
    for bad in ("", "default/", "default/0", "default/x", "gfx_activity", "gfx_activity:", ":gfx_activity", "a:b:c",
                "gfx_activity:average_package_power,", 16, None, ("default",)):
        with pytest.raises(ValueError):
            parse_joint(bad, series, widths)
    with pytest.raises(ValueError):
        parse_joint("default", ("amd_gpu_gfx_activity",))  # none of the default pairs exists


def test_reference_argument_errors():
    from rocmdash.ops.window_joint import window_joint_reference

    rows = np.zeros((64, 3), np.float32)
    window_joint_reference(rows, [(0, 1)], np.arange(31.0))
    for kw in (dict(bounds=np.arange(32.0)), dict(bounds=[2.0, 1.0]), dict(bounds=[]), dict(bounds=np.ones((2, 2))),
               dict(pairs=[(0, 3)]), dict(pairs=[(1, 1)]), dict(pairs=[]), dict(rows=np.zeros(64, np.float32))):
        a = dict(rows=rows, pairs=[(0, 1)], bounds=[1.0, 2.0])
        a.update(kw)
        with pytest.raises(ValueError):
            window_joint_reference(**a)


def test_constants_mirror_the_header():
    from rocmdash.ops import window_joint as wj

    text = open(os.path.join(ROOT, "csrc", "window_joint_plan.h")).read()
    assert int(re.search(r"kMaxJointPairs = (\d+)", text).group(1)) == wj.MAX_PAIRS
    assert int(re.search(r"kMaxJointBuckets = (\d+)", text).group(1)) == wj.MAX_JOINT_BUCKETS
    assert (wj.MAX_JOINT_BUCKETS + 1) ** 2 <= 1024


# ---- kernel resources and the planning header -------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_joint_kernel_has_no_scratch_and_fits_lds(tmp_path):
    """The recipe of test_kernel_resources.py. The table of 8 pairs x 32 x 32 cells is 32 KiB
    and the bounds about 8 KiB: at most 64 KiB per workgroup, so two share a CU. No scratch: the
    by-value argument (the pairs travel in it) is not copied to per-lane memory."""
    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", "window_joint.hip"), "-o", str(tmp_path / "k.o"),
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
    assert any("joint_ring_kernel" in k for k in kernels), res.stderr[-2000:]
    for k, r in kernels.items():
        assert r["ScratchSize [bytes/lane]"] == 0, (k, r)
        assert 32 * 1024 <= r["LDS Size [bytes/block]"] <= LDS_BYTES_PER_WORKGROUP, (k, r)


def test_plan_header_under_sanitizers(tmp_path):
    """tools/joint_plan_check.cpp - a host-only program over the planning header the kernel
    compiles - built with AddressSanitizer and UBSan and run here."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path / "joint_plan_check"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         f"-I{ROOT}/csrc", os.path.join(ROOT, "tools", "joint_plan_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])


# ---- agent without a device -------------------------------------------------------------
def _agent_reference(agent, pairs, bounds):
    from rocmdash.ops.window_joint import window_joint_reference

    starts = np.cumsum([0] + [r.width for r in agent.rings])
    out = []
    for a, b in pairs:
        i = int(np.searchsorted(starts, a, side="right")) - 1
        s, w = int(starts[i]), agent.rings[i].width
        rows, _ = agent.window_host(i)
        out.append(window_joint_reference(np.asarray(rows, np.float32).reshape(-1, w), [(a - s, b - s)], bounds[s:s + w])[0])
    return np.stack(out)


def test_cpu_agent_window_joint_on_a_recording(native):
    from rocmdash.config import SamplerConfig
    from rocmdash.runtime.agent import GpuAgent

    agent = GpuAgent(0, source="replay", replay=CAPTURE, cfg=SamplerConfig(window=128, ring_capacity=512), use_gpu=False)
    try:
        assert agent.dws is None
        index = {s: i for i, s in enumerate(agent.series)}
        defaults = agent.default_joint_pairs()
        assert (index["amd_gpu_gfx_activity"], index["amd_gpu_average_package_power"]) in defaults
        assert (index["amd_gpu_average_package_power"], index["amd_gpu_junction_temperature"]) in defaults
        assert len(defaults) == (4 if "amd_gpu_mfma_utilization" in index else 2)
        empty = agent.window_joint().numpy()
        assert empty.shape == (len(defaults), 17, 17) and empty.dtype == np.int32 and (empty == 0).all()
        agent.prefill(150)
        default = agent.default_bucket_bounds(16)
        custom = np.sort(np.random.default_rng(1).uniform(0, 100, (len(agent.series), 5)).astype(np.float32), axis=1)
        given = [(2, 1), (1, 2), (0, 5)]
        for more in (0, 3):
            for _ in range(more):
                agent.sample()
            for pairs, bounds, p, b in ((None, None, defaults, default), (given, None, given, default),
                                        (given, custom, given, custom)):
                got = agent.window_joint(pairs, bounds).numpy()
                assert got.shape == (len(p), b.shape[1] + 1, b.shape[1] + 1) and got.dtype == np.int32
                np.testing.assert_array_equal(got, _agent_reference(agent, p, b))
            np.testing.assert_array_equal(got[1], got[0].T)
            assert got.sum(axis=(1, 2)).max() == 128
        bad = [dict(pairs=[(1, 1)]), dict(pairs=[]), dict(pairs=[(0, len(agent.series))]), dict(bounds=np.arange(32.0)),
               dict(bounds=[2.0, 1.0])]
        if len(agent.rings) > 1:
            bad.append(dict(pairs=[(0, len(agent.series) - 1)]))
        for kw in bad:
            with pytest.raises(ValueError):
                agent.window_joint(**kw)
    finally:
        agent.close()


# ---- figure -----------------------------------------------------------------------------
_LE_X = [25.0, 50.0, 75.0, 100.0]
_LE_Y = [100.0, 200.0, 400.0, 800.0]
_COUNTS = [[1, 2, 0, 0, 0], [0, 3, 4, 0, 0], [0, 0, 5, 6, 0], [0, 0, 0, 7, 0], [0, 0, 0, 8, 9]]


def test_create_joint_draws_bins_and_leaves_empty_cells_null():
    from rocmdash.viz.figures import create_joint

    fig = create_joint("GPU 0: power vs activity", np.array(_LE_X, np.float32), np.array(_LE_Y, np.float32),
                       np.array(_COUNTS, np.int32), "gfx_activity", "average_package_power", 240)
    doc = json.loads(fig.to_json())  # strict JSON: no NaN
    assert len(doc["data"]) == 1
    t = doc["data"][0]
    assert t["type"] == "heatmap"
    assert t["x"] == [25.0, 50.0, 75.0, 100.0, 125.0]  # the top bin: one bin above the axis maximum
    assert t["y"] == [100.0, 200.0, 400.0, 800.0, 1200.0]
    # z[y bin][x bin] = counts[x bin][y bin]; a cell without a row is null
    assert t["z"] == [[1, None, None, None, None], [2, 3, None, None, None], [None, 4, 5, None, None],
                      [None, None, 6, 7, 8], [None, None, None, None, 9]]
    assert all(isinstance(v, int) for row in t["z"] for v in row if v is not None)
    lay = doc["layout"]
    assert lay["xaxis"]["tickvals"] == t["x"] and lay["xaxis"]["ticktext"] == ["25", "50", "75", "100", "> 100"]
    assert lay["yaxis"]["tickvals"] == t["y"] and lay["yaxis"]["ticktext"] == ["100", "200", "400", "800", "> 800"]
    assert lay["xaxis"]["title"]["text"] == "gfx_activity" and lay["yaxis"]["title"]["text"] == "average_package_power"
    assert lay["height"] == 240 and lay["title"]["text"] == "GPU 0: power vs activity"
    one = json.loads(create_joint("t", [4.0], [0.0], [[1, 0], [0, 2]]).to_json())
    assert one["data"][0]["x"] == [4.0, 8.0] and one["data"][0]["y"] == [0.0, 1.0]
    assert one["data"][0]["z"] == [[1, None], [None, 2]] and "title" not in one["layout"]["xaxis"]
    many = json.loads(create_joint("t", list(range(1, 32)), list(range(1, 32)), np.ones((32, 32), int)).to_json())
    assert len(many["layout"]["xaxis"]["tickvals"]) <= 17 and many["layout"]["yaxis"]["ticktext"][-1] == "> 31"


def test_create_joint_json_matches_plotly():
    go = pytest.importorskip("plotly.graph_objects")
    from rocmdash.viz.figures import create_joint

    xs, ys = _LE_X + [125.0], _LE_Y + [1200.0]
    z = [[1, None, None, None, None], [2, 3, None, None, None], [None, 4, 5, None, None], [None, None, 6, 7, 8],
         [None, None, None, None, 9]]
    ref = go.Figure()
    ref.add_trace(go.Heatmap(x=xs, y=ys, z=z, zmin=0, hoverongaps=False, colorbar=dict(title=dict(text="rows"))))
    ref.update_layout(title=dict(text="GPU 0"),
                      xaxis=dict(tickmode="array", tickvals=xs, ticktext=["25", "50", "75", "100", "> 100"], title=dict(text="a")),
                      yaxis=dict(tickmode="array", tickvals=ys, ticktext=["100", "200", "400", "800", "> 800"], title=dict(text="b")),
                      margin=dict(l=40, r=20, t=40, b=40), height=260, showlegend=False)
    ours = create_joint("GPU 0", _LE_X, _LE_Y, _COUNTS, "a", "b")
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


def test_exporter_serves_joint_json_and_404_without(native, monkeypatch):
    """A synthetic source without a GPU: /joint is the documented strict JSON; off (the default)
    it is a 404 with a hint; the joint histograms never reach /metrics, and /trend and /heatmap
    stay off."""
    import torch

    from rocmdash.prom.exporter import Exporter

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # agents on the CPU, wherever this runs
    monkeypatch.delenv("ROCMDASH_WINDOW_JOINT", raising=False)
    src = _local_source(window_joint="default/5")
    exp = Exporter(src, hostname="n1")
    try:
        agent = src.agents[0]
        assert agent.dws is None and src.joint[1] == 5 and src.joint[0] == agent.default_joint_pairs()
        assert len(src.joint[0]) == 4
        agent.prefill(40)
        exp.serve("127.0.0.1", 0)
        code, ctype, body = _get(exp.port, "/joint?x=1")
        assert code == 200 and ctype == "application/json"
        doc = _strict(body)
        assert set(doc) == {"buckets", "pairs", "gpus"}
        assert doc["buckets"] == 5
        assert doc["pairs"] == [[src.series[a], src.series[b]] for a, b in src.joint[0]]
        assert doc["pairs"][0] == ["amd_gpu_mfma_utilization", "amd_gpu_hbm_read_bandwidth"]
        assert list(doc["gpus"]) == [agent.info.gpu_id]
        per = doc["gpus"][agent.info.gpu_id]
        want = agent.window_joint(src.joint[0], src.joint_bounds).numpy()
        assert len(per) == 4
        for k, ((a, b), m) in enumerate(zip(src.joint[0], per)):
            assert set(m) == {"x", "y", "le_x", "le_y", "counts", "rows"}
            assert [m["x"], m["y"]] == doc["pairs"][k]
            assert m["le_x"] == [float(v) for v in src.joint_bounds[a]] and len(m["le_x"]) == 5
            assert m["le_y"] == [float(v) for v in src.joint_bounds[b]] and len(m["le_y"]) == 5
            assert len(m["counts"]) == 6 and all(len(c) == 6 for c in m["counts"])
            assert all(isinstance(v, int) for c in m["counts"] for v in c)
            assert m["counts"] == want[k].tolist()
            assert isinstance(m["rows"], int) and m["rows"] == sum(map(sum, m["counts"]))
        # (the samplers may have pushed a row or two before they were stopped)
        assert 40 <= per[2]["rows"] == agent.rings[0].head < 56
        metrics = _get(exp.port, "/metrics")[2].decode()
        assert "joint" not in metrics
        assert _get(exp.port, "/heatmap")[0] == 404 and _get(exp.port, "/trend")[0] == 404
    finally:
        exp.close()

    src = _local_source()
    exp = Exporter(src, hostname="n1")
    try:
        assert src.joint is None and src.joint_bounds is None
        exp.serve("127.0.0.1", 0)
        code, _, body = _get(exp.port, "/joint")
        assert code == 404 and b"--window-joint" in body
        assert _get(exp.port, "/metrics")[0] == 200
        snap, _ = src.collect()
        assert snap.window_joint is None and snap.window_joint_pairs is None
    finally:
        exp.close()


def test_metrics_are_byte_identical_with_the_joint_on_and_off(native):
    """The same snapshot with and without joint histograms renders the same /metrics text."""
    import copy

    from rocmdash.prom.exporter import SyntheticSource, render_joint
    from rocmdash.prom.exposition import render_snapshot

    snap, _ = SyntheticSource(2, seed=3).collect()
    snap.window_series = tuple(snap.columns[:3])
    snap.window = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    off = render_snapshot(snap, hostname="n1")
    assert render_joint(snap) is None
    on = copy.copy(snap)
    on.window_joint = np.zeros((2, 2, 5, 5), np.int32)
    on.window_joint[:, 0, 1, 2] = 7
    on.window_joint[:, 1, 2, 1] = 7
    on.window_joint_pairs = ((0, 2), (2, 0))
    on.window_joint_bounds = np.broadcast_to(np.array([1, 2, 3, 4], np.float32), (2, 3, 4))
    assert render_snapshot(on, hostname="n1") == off
    doc = _strict(render_joint(on))
    assert doc["buckets"] == 4 and doc["pairs"] == [[snap.columns[0], snap.columns[2]], [snap.columns[2], snap.columns[0]]]
    m = doc["gpus"][snap.gpu_ids[1]][0]
    assert m["le_x"] == [1.0, 2.0, 3.0, 4.0] and m["rows"] == 7 and m["counts"][1] == [0, 0, 7, 0, 0]


def test_exporter_option_from_the_environment_and_refusals(native, monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCMDASH_WINDOW_JOINT", "gfx_activity:average_package_power,average_package_power:gfx_activity/4")
    src = _local_source()
    try:
        assert src.joint == ([(1, 2), (2, 1)], 4)
        src.agents[0].prefill(70)
        snap, _ = src.collect()
        assert snap.window_joint.shape == (1, 2, 5, 5) and snap.window_joint.dtype == np.int32
        assert snap.window_joint_pairs == ((1, 2), (2, 1)) and snap.window_joint_bounds.shape == (1, len(src.series), 4)
        np.testing.assert_array_equal(snap.window_joint[0, 1], snap.window_joint[0, 0].T)
        assert snap.window_joint[0, 0].sum() == 64
    finally:
        src.close()
    for bad, msg in (("gfx_activity:mfma_utilization", "spans rings"), ("default/32", "1 to 31 buckets"),
                     ("gfx_activity:warp_speed", "unknown metric"), ("gfx_activity", "metricA:metricB")):
        monkeypatch.setenv("ROCMDASH_WINDOW_JOINT", bad)
        with pytest.raises(ValueError, match=msg):
            _local_source()


def test_exporter_command_line_rejects_a_bad_joint(capsys):
    from rocmdash.prom.exporter import main

    for bad, msg in (("gfx_activity:mfma_utilization", "no common row number"), ("default/32", "1 to 31"),
                     ("gfx_activity:warp_speed", "unknown metric")):
        with pytest.raises(SystemExit):
            main(["--window-joint", bad])
        err = capsys.readouterr().err
        assert "--window-joint" in err and msg in err


# ---- page -------------------------------------------------------------------------------
def test_page_joint_figures_only_with_a_joint():
    from rocmdash.prom.exporter import SyntheticSource
    from rocmdash.ui.page import window_joint_figures

    snap, _ = SyntheticSource(2, seed=1).collect()
    assert window_joint_figures(snap, snap.gpu_ids) is None  # no joint histograms: the page is as it was
    snap.window_series = ("amd_gpu_gfx_activity", "amd_gpu_average_package_power", "other")
    snap.window_joint = np.zeros((2, 2, 5, 5), np.int32)
    snap.window_joint[:, 0, 1, 3] = 4
    snap.window_joint[:, 1, 3, 1] = 4
    snap.window_joint_pairs = ((0, 1), (2, 0))
    snap.window_joint_bounds = np.broadcast_to(np.array([25, 50, 75, 100], np.float32), (2, 3, 4))
    figs = window_joint_figures(snap, [snap.gpu_ids[1]])
    gid = snap.gpu_ids[1]
    assert [k for k, _ in figs] == [f"plot_joint_gfx_activity_average_package_power_{gid}_", f"plot_joint_other_gfx_activity_{gid}_"]
    doc = json.loads(figs[0][1].to_json())
    t = doc["data"][0]
    assert t["type"] == "heatmap" and t["z"][3][1] == 4 and sum(v is not None for row in t["z"] for v in row) == 1
    assert doc["layout"]["xaxis"]["title"]["text"] == "gfx_activity"
    assert len(window_joint_figures(snap, snap.gpu_ids)) == 4
