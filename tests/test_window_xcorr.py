"""Window cross-correlation (rocmdash.ops.window_xcorr) without a GPU: the reference against a
triple loop in Python ints, its identities, the coefficient per lag and the lag rule, the
option's parsing, the planning header under sanitizers, the exporter's /xcorr and lag gauges,
the figure, the agent's CPU path and the kernel's compile-time resources."""

import json
import os
import re
import shutil
import subprocess
import urllib.error
import urllib.request

import numpy as np
import pytest

from _window_xcorr import assert_mirror, rows as _rows, scale as _scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURE = os.path.join(ROOT, "tests", "fixtures", "mi355x_capture.npz")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_BYTES_PER_WORKGROUP = 64 * 1024


# ---- reference --------------------------------------------------------------------------
def _brute(rows, pairs, scale, L, span):
    """The table of the semantics as a triple loop over (pair, k, t) in Python ints."""
    from rocmdash.ops.window_autocorr import quantise

    N = min(len(rows), span)
    q, v = quantise(rows[len(rows) - N:], scale)
    q, v = q.tolist(), v.tolist()
    out = [[[0] * 6 for _ in range(2 * L + 1)] for _ in pairs]
    for i, (a, b) in enumerate(pairs):
        for k in range(-L, L + 1):
            w = out[i][L + k]
            for t in range(N):
                if not 0 <= t + k < N:
                    continue
                w[0] += v[t][a] * v[t + k][b]
                w[1] += q[t][a] * v[t + k][b]
                w[2] += v[t][a] * q[t + k][b]
                w[3] += q[t][a] * q[t + k][b]
                w[4] += q[t][a] ** 2 * v[t + k][b]
                w[5] += v[t][a] * q[t + k][b] ** 2
    return np.array(out, dtype=np.int64).reshape(len(pairs), 2 * L + 1, 6)


@pytest.mark.parametrize("L", [1, 5, 70])
@pytest.mark.parametrize("n", [0, 1, 2, 70, 200])
def test_reference_against_the_triple_loop(n, L):
    from rocmdash.ops.window_xcorr import window_xcorr_reference

    pairs = [(0, 2), (2, 0), (1, 0)]
    rows = np.ascontiguousarray(_rows(n * 100 + L, 3, n, nan=0.05).T)
    for span in (None, 64):  # 64 cuts the windows of 70 and 200 rows
        got = window_xcorr_reference(rows, pairs, _scale(3), L, span)
        assert got.dtype == np.int64 and got.shape == (3, 2 * L + 1, 6)
        np.testing.assert_array_equal(got, _brute(rows, pairs, _scale(3), L, span or 65536))
    if n == 200:
        assert window_xcorr_reference(rows, pairs, _scale(3), L, 64)[0, L, 0] <= 64


def test_identities():
    """(b, a) at lag k is (a, b) at lag -k with Sx <-> Sy and Sxx <-> Syy; without NaNs n_k = N -
    |k|, lags with |k| >= N are zero, and lag 0 agrees with the autocorrelation of series a."""
    from rocmdash.ops.window_autocorr import window_autocorr_reference
    from rocmdash.ops.window_xcorr import window_xcorr_reference

    L = 70
    for n, nan in ((200, 0.05), (200, 0.0), (40, 0.0)):
        rows = np.ascontiguousarray(_rows(n, 4, n, nan=nan).T)
        out = window_xcorr_reference(rows, [(0, 3), (3, 0), (1, 2), (2, 1)], _scale(4), L)
        assert_mirror(out[0], out[1])
        assert_mirror(out[2], out[3])
        if not nan:
            k = np.abs(np.arange(-L, L + 1))
            assert (out[:, :, 0] == np.maximum(n - k, 0)[None]).all()
            assert (out[:, k >= n] == 0).all()
            auto = window_autocorr_reference(rows, _scale(4), L)
            for i, (a, b) in enumerate([(0, 3), (3, 0), (1, 2), (2, 1)]):
                assert out[i, L, 1] == auto[a, 0, 1] and out[i, L, 4] == auto[a, 0, 3]  # Sx_0, Sxx_0 of series a
                assert out[i, L, 2] == auto[b, 0, 1] and out[i, L, 5] == auto[b, 0, 3]
    for bad in (dict(pairs=[(0, 0)]), dict(pairs=[]), dict(pairs=[(0, 1)] * 9), dict(pairs=[(0, 4)]), dict(L=0), dict(L=1025),
                dict(span=100)):
        kw = dict(pairs=[(0, 1)], L=4, span=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            window_xcorr_reference(rows, kw["pairs"], _scale(4), kw["L"], kw["span"])


# ---- coefficient and lag ----------------------------------------------------------------
def _sums(a, b, L, scale=4095.0 / 100.0):
    from rocmdash.ops.window_xcorr import window_xcorr_reference

    rows = np.stack([np.asarray(a, np.float32), np.asarray(b, np.float32)], axis=1)
    return window_xcorr_reference(rows, [(0, 1)], np.full(2, scale, np.float32), L, 1 << 16)[0]


def _delayed(a, d):
    """b[t] = a[t - d], the rows without a source held at a's nearest end."""
    t = np.clip(np.arange(len(a)) - d, 0, len(a) - 1)
    return a[t]


def _walk(rng, n=4096):
    a = np.cumsum(rng.normal(0, 1, n))
    return 10.0 + 80.0 * (a - a.min()) / (a.max() - a.min())


def test_cross_correlogram_edges():
    from rocmdash.ops.window_xcorr import cross_correlogram

    rng = np.random.default_rng(1)
    a = rng.uniform(10, 90, 512)
    L = 16
    const = cross_correlogram(_sums(a, np.full(512, 40.0), L))
    assert const.shape == (2 * L + 1,) and np.isnan(const).all()  # a constant series: db == 0 at every lag
    assert np.isnan(cross_correlogram(_sums(np.full(512, 40.0), a, L))).all()
    d = 5
    r = cross_correlogram(_sums(a[d:], a[:-d], L))  # b[t] = a'[t - d] exactly, over the samples that pair up
    assert r[L + d] == 1.0 and np.nanmax(r) == 1.0 and (np.abs(r[np.arange(2 * L + 1) != L + d]) < 0.5).all()
    neg = cross_correlogram(_sums(a, 100.0 - a, L, scale=40.0))  # 40 q per unit: 100 - a quantises to 4000 - qa, exactly
    assert neg[L] == -1.0
    short = cross_correlogram(_sums(a[:20], a[:20] + 1.0, L))
    n = 20 - np.abs(np.arange(-L, L + 1))
    assert np.isnan(short[2 * n < 20]).all() and np.isfinite(short[2 * n >= 20]).all() and np.isnan(short).any()
    both = cross_correlogram(np.stack([_sums(a, 100.0 - a, L), _sums(a, a, L)]))
    assert both.shape == (2, 2 * L + 1) and both[1, L] == 1.0
    assert np.isnan(cross_correlogram(np.zeros((2 * L + 1, 6), np.int64))).all()
    with pytest.raises(ValueError):
        cross_correlogram(np.zeros((4, 6), np.int64))


@pytest.mark.parametrize("d", [0, 3, 40, -17])
def test_pick_lag_finds_the_delay(d):
    """b[t] = a[t - d] + noise with a a random walk of 4096 rows: exactly d."""
    from rocmdash.ops.window_xcorr import cross_correlogram, pick_lag

    rng = np.random.default_rng(100 + abs(d))
    a = _walk(rng)
    b = _delayed(a, d) + rng.normal(0, 0.5, len(a))
    lag, r = pick_lag(cross_correlogram(_sums(a, b, 64)))
    assert lag == d and r > 0.9


def test_pick_lag_negative_coupling_none_and_periodic():
    from rocmdash.ops.window_xcorr import cross_correlogram, pick_lag

    rng = np.random.default_rng(7)
    a = _walk(rng)
    lag, r = pick_lag(cross_correlogram(_sums(a, 100.0 - _delayed(a, 6) + rng.normal(0, 0.5, len(a)), 64)))
    assert lag == 6 and r < -0.9  # a negative coupling: the signed coefficient
    noise = cross_correlogram(_sums(rng.uniform(0, 100, 4096), rng.uniform(0, 100, 4096), 64))
    assert pick_lag(noise) == (None, None) and np.nanmax(np.abs(noise)) < 0.2
    t = np.arange(4096)
    sq = lambda shift: np.where(((t - shift) % 50) < 25, 80.0, 20.0) + rng.normal(0, 3.0, len(t))  # noqa: E731
    ccf = cross_correlogram(_sums(sq(0), sq(7), 100))
    lag, r = pick_lag(ccf)
    assert lag == 7 and r > 0.9  # not 57, not -43: near-equal peaks one period apart, the nearest to zero wins
    assert ccf[100 + 57] > 0.9 and ccf[100 - 43] > 0.9
    # the rule itself, on hand-made coefficients (L = 4)
    nan = float("nan")
    assert pick_lag([0, .2, .9, .2, 0, .2, .9, .2, 0]) == (2, .9)  # -2 and +2 tie: +k
    assert pick_lag([0, .2, -.95, .2, 0, .2, .9, .2, 0]) == (-2, -.95)  # the larger |r| first
    assert pick_lag([.99, .2, .1, .2, .3, .2, .1, .2, .99]) == (None, None)  # the ends are no candidates; 0.3 < 0.5
    assert pick_lag([0, .1, .2, .6, nan, .2, .1, 0, 0]) == (None, None)  # a neighbour without a coefficient
    assert pick_lag([0, .1, .7, .1, 0, .1, .74, .1, 0], tolerance=0.01) == (2, .74)
    assert pick_lag([0, .1, .7, .1, 0, .1, .1, .74, 0]) == (-2, .7)  # within the tolerance: the smaller |k|
    assert pick_lag([nan] * 9) == (None, None)


# ---- option -----------------------------------------------------------------------------
def test_parse_and_check_xcorr():
    from rocmdash.ops import window_xcorr as wx
    from rocmdash.ops.window_joint import DEFAULT_PAIRS, PREFIX

    smi = [PREFIX + m for m in ("gfx_activity", "average_package_power", "junction_temperature")]
    ctr = [PREFIX + m for m in ("mfma_utilization", "hbm_read_bandwidth", "hbm_write_bandwidth")]
    series, widths = smi + ctr, (3, 3)
    want = [(series.index(PREFIX + a), series.index(PREFIX + b)) for a, b in DEFAULT_PAIRS]
    assert wx.parse_xcorr("default", series, widths) == (want, 255, 65536)
    assert wx.parse_xcorr("default", smi) == ([(0, 1), (1, 2)], 255, 65536)  # only the pairs whose series exist
    assert wx.parse_xcorr(" default/64 ", series, widths) == (want, 64, 65536)
    assert wx.parse_xcorr("gfx_activity:junction_temperature/8/4096", series, widths) == ([(0, 2)], 8, 4096)
    assert wx.parse_xcorr("amd_gpu_gfx_activity:junction_temperature, hbm_read_bandwidth : amd_gpu_mfma_utilization/1024",
                          series, widths) == ([(0, 2), (4, 3)], 1024, 65536)
    nine = ",".join(["gfx_activity:junction_temperature"] * 9)
    for bad in ("nope:gfx_activity", "gfx_activity:gfx_activity", nine, "default/0", "default/1025", "default/8/100",
                "default/x", "default/8/4096/2", "gfx_activity", "", "default/", 5, None):
        with pytest.raises(ValueError):
            wx.parse_xcorr(bad, series, widths)
    with pytest.raises(ValueError, match="spans rings 0 and 1: rows of different rings have no common row number"):
        wx.parse_xcorr("gfx_activity:mfma_utilization", series, widths)
    assert wx.check_xcorr(1, 64, 4096) == (1, 64) and wx.check_xcorr(63, 64, 64) == (63, 64) and wx.check_xcorr(255) == (255, 65536)
    for L, span, window in ((64, 64, 4096), (64, 4096, 64), (0, 64, 64), (1025, None, None), (8, 100, None), (8, 32, None)):
        with pytest.raises(ValueError):
            wx.check_xcorr(L, span, window)


def test_constants_mirror_the_header():
    from rocmdash.ops import window_autocorr as wa, window_joint as wj, window_xcorr as wx

    text = "".join(open(os.path.join(ROOT, "csrc", f)).read() for f in ("window_xcorr_plan.h", "window_lag_dev.h", "window_xcorr.hip"))

    def const(name):
        m = re.search(rf"constexpr \w+ {name} = (?:(\d+)u?|1u << (\d+));", text)
        assert m, f"{name} is no plain integer constant any more"
        return int(m.group(1)) if m.group(1) else 1 << int(m.group(2))

    want = {"kMaxXcorrPairs": wj.MAX_PAIRS, "kXcorrWords": wx.WORDS, "kXcorrGroupPairs": wx.GROUP_PAIRS,
            "kXcorrLagBlock": wx.LAG_BLOCK, "kXcorrLagTile": wx.LAG_TILE, "kXcorrChunk": wa.CHUNK, "kMaxXcorrLags": wa.MAX_LAGS,
            "kFold": wa.FOLD}
    assert {k: const(k) for k in want} == want
    assert wx.MAX_LAGS == wa.MAX_LAGS and wx.MAX_PAIRS == wj.MAX_PAIRS and wx.DEFAULT_LAGS == wx.LAG_BLOCK - 1
    assert wa.FOLD * wa.Q_MAX ** 2 < 2 ** 31 and wa.Q_MAX ** 2 * wa.MAX_SPAN < 2 ** 44 and wa.Q_MAX * wa.MAX_SPAN < 2 ** 32
    assert wx.quantise is wa.quantise and wx.check_scale is wa.check_scale and wx.default_scale is wa.default_scale
    assert wx.check_pairs is wj.check_pairs


# ---- planning header and kernel resources -----------------------------------------------
def test_plan_header_under_sanitizers(tmp_path):
    """tools/xcorr_plan_check.cpp - a host-only program over the planning header the kernel
    compiles - built with AddressSanitizer and UBSan and run here."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path / "xcorr_plan_check"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         f"-I{ROOT}/csrc", os.path.join(ROOT, "tools", "xcorr_plan_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_xcorr_kernel_has_no_scratch_and_fits_lds(tmp_path):
    """The recipe of test_autocorr_kernel_has_no_scratch_and_fits_lds for window_xcorr.hip, with
    the LDS of a workgroup within 64 KB."""
    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", "window_xcorr.hip"), "-o", str(tmp_path / "k.o"),
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
    assert any("xcorr_ring_kernel" in k for k in kernels), res.stderr[-2000:]
    for k, r in kernels.items():
        assert r["ScratchSize [bytes/lane]"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] <= LDS_BYTES_PER_WORKGROUP, (k, r)


# ---- agent without a device -------------------------------------------------------------
def _agent_reference(agent, pairs, scale, L, span):
    from rocmdash.ops.window_xcorr import window_xcorr_reference

    starts = np.cumsum([0] + [r.width for r in agent.rings])
    out = []
    for a, b in pairs:
        i = int(np.searchsorted(starts, a, side="right")) - 1
        s, w = int(starts[i]), agent.rings[i].width
        rows, _ = agent.window_host(i)
        out.append(window_xcorr_reference(np.asarray(rows, np.float32).reshape(-1, w), [(a - s, b - s)], scale[s:s + w], L, span)[0])
    return np.stack(out)


def test_cpu_agent_window_xcorr_on_a_recording(native):
    from rocmdash.config import SamplerConfig
    from rocmdash.runtime.agent import GpuAgent

    agent = GpuAgent(0, source="replay", replay=CAPTURE, cfg=SamplerConfig(window=128, ring_capacity=512), use_gpu=False)
    try:
        assert agent.dws is None
        scale = agent.default_autocorr_scale()
        pairs = agent.default_joint_pairs()
        assert 1 <= len(pairs) <= 8
        empty = agent.window_xcorr(L=16).numpy()
        assert empty.shape == (len(pairs), 33, 6) and empty.dtype == np.int64 and (empty == 0).all()
        agent.prefill(150)
        custom = np.full(len(agent.series), 3.0, np.float32)
        mirrored = [pairs[0], pairs[0][::-1]]
        for p, L, span, sc, want_sc in ((None, 16, None, None, scale), (None, 40, 64, None, scale), (mirrored, 16, None, custom, custom)):
            got = agent.window_xcorr(p, L, span, sc).numpy()
            np.testing.assert_array_equal(got, _agent_reference(agent, p or pairs, want_sc, L, span))
            assert got[:, L, 0].max() == min(128, span or 128)
        assert_mirror(got[0], got[1])
        widths = [r.width for r in agent.rings]
        bad = [dict(L=0), dict(L=128), dict(L=8, span=100), dict(L=8, scale=np.zeros(len(agent.series), np.float32)),
               dict(L=8, pairs=[(0, 0)]), dict(L=8, pairs=[])]
        if len(widths) > 1:
            bad.append(dict(L=8, pairs=[(0, widths[0])]))  # across rings
        for kw in bad:
            with pytest.raises(ValueError):
                agent.window_xcorr(**kw)
    finally:
        agent.close()


# ---- figure -----------------------------------------------------------------------------
def test_create_xcorr_json():
    from rocmdash.viz.figures import create_xcorr

    nan = float("nan")
    fig = create_xcorr("GPU 0: temp after power", [nan, 0.25, -0.5, 0.75, 0.5], 1, "power", "temp")
    doc = json.loads(fig.to_json())
    assert [t["name"] for t in doc["data"]] == ["temp after power", "lag 1"]
    assert doc["data"][0]["x"] == [-2, -1, 0, 1, 2] and doc["data"][0]["y"] == [None, 0.25, -0.5, 0.75, 0.5]
    assert doc["data"][1]["x"] == [1] and doc["data"][1]["y"] == [0.75] and doc["data"][1]["mode"] == "markers"
    assert doc["layout"]["xaxis"]["title"]["text"] == "lag (samples)" and doc["layout"]["yaxis"]["range"] == [-1, 1]
    assert doc["layout"]["shapes"][0]["x0"] == 0 and doc["layout"]["shapes"][0]["x1"] == 0  # the zero line
    assert json.loads(fig.to_plotly().to_json()) == doc
    one = json.loads(create_xcorr("t", [0.1, 1.0, 0.1]).to_json())
    assert len(one["data"]) == 1 and one["data"][0]["x"] == [-1, 0, 1]
    neg = json.loads(create_xcorr("t", [0.1, 0.2, 0.1, -0.9, nan], -2).to_json())
    assert neg["data"][1]["x"] == [-2] and neg["data"][1]["y"] == [0.1]


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


def test_exporter_serves_xcorr_json_and_404_without(native, monkeypatch):
    """A synthetic source without a GPU: /xcorr is the documented strict JSON with null for NaN
    and for "no lag"; off (the default) it is a 404 with a hint, the snapshot carries nothing and
    /metrics is byte-identical to that of a source that never heard of the option."""
    import torch

    from rocmdash.ops.window_xcorr import cross_correlogram, pick_lag
    from rocmdash.prom.exporter import Exporter
    from rocmdash.prom.exposition import render_snapshot

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # agents on the CPU, wherever this runs
    monkeypatch.delenv("ROCMDASH_WINDOW_XCORR", raising=False)
    src = _local_source(window_xcorr="default/20/64")
    exp = Exporter(src, hostname="n1")
    try:
        agent = src.agents[0]
        pairs = agent.default_joint_pairs()
        assert agent.dws is None and src.xcorr == (pairs, 20, 64)
        agent.prefill(70)
        exp.serve("127.0.0.1", 0)
        code, ctype, body = _get(exp.port, "/xcorr?x=1")
        assert code == 200 and ctype == "application/json"
        doc = _strict(body)
        assert set(doc) == {"lags", "span", "pairs", "gpus"}
        assert doc["lags"] == 20 and doc["span"] == 64
        assert doc["pairs"] == [[src.series[a], src.series[b]] for a, b in pairs]
        assert list(doc["gpus"]) == [agent.info.gpu_id]
        per = doc["gpus"][agent.info.gpu_id]
        want = agent.window_xcorr(pairs, 20, 64, src.xcorr_scale).numpy()
        assert len(per) == len(pairs)
        for k, d in enumerate(per):
            assert set(d) == {"x", "y", "ccf", "pairs", "lag_samples", "correlation"}
            assert [d["x"], d["y"]] == doc["pairs"][k]
            assert d["pairs"] == want[k, :, 0].tolist() and all(isinstance(v, int) for v in d["pairs"])
            ccf = cross_correlogram(want[k])
            assert len(d["ccf"]) == 41 and d["ccf"] == [None if v != v else float(v) for v in ccf]
            lag, r = pick_lag(ccf)
            assert d["lag_samples"] == lag and d["correlation"] == r
        assert _get(exp.port, "/joint")[0] == 404 and _get(exp.port, "/autocorr")[0] == 404
    finally:
        exp.close()

    src = _local_source()
    exp = Exporter(src, hostname="n1")
    try:
        assert src.xcorr is None and src.xcorr_scale is None
        exp.serve("127.0.0.1", 0)
        code, _, body = _get(exp.port, "/xcorr")
        assert code == 404 and b"--window-xcorr" in body
        metrics = _get(exp.port, "/metrics")
        assert metrics[0] == 200 and b"rocmdash_window_lag" not in metrics[2]
        snap, _ = src.collect()
        assert snap.window_xcorr is None and snap.window_xcorr_pairs is None and snap.window_xcorr_span is None
        assert "rocmdash_window_lag" not in render_snapshot(snap, hostname="n1")
    finally:
        exp.close()


def test_lag_gauges_only_where_there_is_a_lag():
    """/metrics of a snapshot with sums: the two families for the pairs that have a lag only;
    without sums the text is byte-identical to what it was."""
    import copy

    from rocmdash.prom.exporter import SyntheticSource, render_xcorr
    from rocmdash.prom.exposition import render_snapshot

    snap, _ = SyntheticSource(2, seed=3).collect()
    snap.window_series = tuple(snap.columns[:3])
    snap.window = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    off = render_snapshot(snap, hostname="n1")
    assert render_xcorr(snap) is None and "rocmdash_window_lag" not in off
    rng = np.random.default_rng(2)
    a = _walk(rng)
    follows = _sums(a, 100.0 - _delayed(a, 9) + rng.normal(0, 0.5, len(a)), 32)  # y follows x by 9, inverted
    leads = _sums(a, _delayed(a, -4) + rng.normal(0, 0.5, len(a)), 32)
    nothing = _sums(rng.uniform(0, 100, 4096), rng.uniform(0, 100, 4096), 32)
    on = copy.copy(snap)
    on.window_xcorr = np.stack([np.stack([follows, nothing, leads]), np.stack([nothing, nothing, nothing])])
    on.window_xcorr_pairs, on.window_xcorr_span = ((0, 1), (1, 2), (2, 0)), 4096
    text = render_snapshot(on, hostname="n1")
    added = [ln for ln in text.splitlines() if ln not in off.splitlines()]
    assert "\n".join(ln for ln in text.splitlines() if ln not in added) == off.rstrip("\n")
    values = [ln for ln in added if not ln.startswith("#")]
    assert len(values) == 4 and all("rocmdash_window_lag_" in ln for ln in values)
    g0, g1 = snap.gpu_ids
    c = snap.columns
    got = {}
    for ln in values:
        key = (ln.split("{")[0],) + tuple(re.search(rf'{lab}="([^"]*)"', ln).group(1) for lab in ("gpu_id", "x", "y"))
        got[key] = float(ln.rsplit(" ", 1)[1])
    assert set(got) == {(f, g0, x, y) for f in ("rocmdash_window_lag_samples", "rocmdash_window_lag_correlation")
                        for x, y in ((c[0], c[1]), (c[2], c[0]))}
    assert got[("rocmdash_window_lag_samples", g0, c[0], c[1])] == 9 and got[("rocmdash_window_lag_samples", g0, c[2], c[0])] == -4
    assert got[("rocmdash_window_lag_correlation", g0, c[0], c[1])] < -0.9
    assert got[("rocmdash_window_lag_correlation", g0, c[2], c[0])] > 0.9
    doc = _strict(render_xcorr(on))
    assert doc["lags"] == 32 and doc["span"] == 4096 and doc["pairs"] == [[c[0], c[1]], [c[1], c[2]], [c[2], c[0]]]
    assert [d["lag_samples"] for d in doc["gpus"][g0]] == [9, None, -4] and doc["gpus"][g0][1]["correlation"] is None
    assert [d["lag_samples"] for d in doc["gpus"][g1]] == [None, None, None]


def test_exporter_option_from_the_environment_and_refusals(native, monkeypatch, capsys):
    import torch

    from rocmdash.prom.exporter import main

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCMDASH_WINDOW_XCORR", "gfx_activity:average_package_power/16")
    src = _local_source()
    try:
        a, b = src.series.index("amd_gpu_gfx_activity"), src.series.index("amd_gpu_average_package_power")
        assert src.xcorr == ([(a, b)], 16, 65536)
        src.agents[0].prefill(70)
        snap, _ = src.collect()
        assert snap.window_xcorr.shape == (1, 1, 33, 6) and snap.window_xcorr.dtype == np.int64
        assert snap.window_xcorr_pairs == ((a, b),) and snap.window_xcorr_span == 65536 and snap.window_xcorr[0, 0, 16, 0] == 64
    finally:
        src.close()
    # 64 lags need more than the window's 64 rows; the default 255 lags too
    for bad in ("default/0", "default/2000", "default/8/100", "default/64", "default", "abc", "nope:gfx_activity/8",
                "gfx_activity:gfx_activity/8", "gfx_activity:mfma_utilization/8"):
        monkeypatch.setenv("ROCMDASH_WINDOW_XCORR", bad)
        with pytest.raises(ValueError):
            _local_source()
    monkeypatch.delenv("ROCMDASH_WINDOW_XCORR")
    for bad in ("default/0", "default/8/100", "default/x", "nope:gfx_activity", "gfx_activity:mfma_utilization"):
        with pytest.raises(SystemExit):
            main(["--window-xcorr", bad])
        assert "--window-xcorr" in capsys.readouterr().err


# ---- page -------------------------------------------------------------------------------
def test_page_xcorr_figures_only_with_sums():
    from rocmdash.prom.exporter import SyntheticSource
    from rocmdash.ui.page import window_xcorr_figures

    snap, _ = SyntheticSource(2, seed=1).collect()
    assert window_xcorr_figures(snap, snap.gpu_ids) is None  # no sums: the page is as it was
    snap.window_series = ("amd_gpu_average_package_power", "amd_gpu_junction_temperature")
    rng = np.random.default_rng(5)
    a = _walk(rng, 2048)
    sums = np.stack([_sums(a, _delayed(a, 12) + rng.normal(0, 0.5, len(a)), 32), _sums(a, np.full(len(a), 50.0), 32)])
    snap.window_xcorr, snap.window_xcorr_pairs, snap.window_xcorr_span = np.stack([sums, sums]), ((0, 1), (1, 0)), 2048
    figs = window_xcorr_figures(snap, [snap.gpu_ids[1]])
    g = snap.gpu_ids[1]
    assert [k for k, _ in figs] == [f"plot_xcorr_average_package_power_junction_temperature_{g}_",
                                    f"plot_xcorr_junction_temperature_average_package_power_{g}_"]
    doc = json.loads(figs[0][1].to_json())
    assert doc["data"][1]["x"] == [12] and doc["data"][0]["x"][0] == -32 and len(doc["data"][0]["y"]) == 65
    flat = json.loads(figs[1][1].to_json())
    assert len(flat["data"]) == 1 and flat["data"][0]["y"] == [None] * 65  # a constant series: no coefficient, no marker
