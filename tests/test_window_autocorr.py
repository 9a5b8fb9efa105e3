"""Window autocorrelation (rocmdash.ops.window_autocorr) without a GPU: the reference against a
triple loop in Python ints, the quantisation rule, the correlogram and the period rule, the
option's parsing, the exporter's /autocorr and period gauges, the figure, the agent's CPU path
and the kernel's compile-time resources."""

import json
import os
import re
import shutil
import subprocess
import urllib.error
import urllib.request

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURE = os.path.join(ROOT, "tests", "fixtures", "mi355x_capture.npz")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_BYTES_PER_CU = 160 * 1024


# ---- reference --------------------------------------------------------------------------
def _brute(rows, scale, L, span):
    """The table of the semantics as a triple loop over Python ints."""
    from rocmdash.ops.window_autocorr import quantise

    N = min(len(rows), span)
    q, v = quantise(rows[len(rows) - N:], scale)
    q, v = q.tolist(), v.tolist()
    S = rows.shape[1]
    out = [[[0, 0, 0, 0] for _ in range(L + 1)] for _ in range(S)]
    for s in range(S):
        for k in range(L + 1):
            for t in range(max(N - k, 0)):
                out[s][k][0] += v[t][s] * v[t + k][s]
                out[s][k][1] += q[t][s] * v[t + k][s]
                out[s][k][2] += v[t][s] * q[t + k][s]
                out[s][k][3] += q[t][s] * q[t + k][s]
    return np.array(out, dtype=np.int64).reshape(S, L + 1, 4)


@pytest.mark.parametrize("n,L,span", [(0, 3, 64), (1, 3, 64), (2, 5, 64), (40, 7, 64), (90, 12, 64), (7, 9, 64)])
def test_reference_against_a_triple_loop(n, L, span):
    from rocmdash.ops.window_autocorr import window_autocorr_reference

    rng = np.random.default_rng(n + L)
    rows = rng.uniform(-10, 120, (n, 3)).astype(np.float32)
    rows[rng.random((n, 3)) < 0.15] = np.nan
    scale = np.array([40.95, 1.0, 7.5], np.float32)
    got = window_autocorr_reference(rows, scale, L, span)
    assert got.dtype == np.int64 and got.shape == (3, L + 1, 4)
    np.testing.assert_array_equal(got, _brute(rows, scale, L, span))


def test_reference_identities():
    from rocmdash.ops.window_autocorr import quantise, window_autocorr_reference

    rng = np.random.default_rng(4)
    rows = rng.uniform(0, 100, (300, 2)).astype(np.float32)
    scale = np.full(2, np.float32(40.95), np.float32)
    L, N = 20, 256
    out = window_autocorr_reference(rows, scale, L, N)
    q, _ = quantise(rows[-N:], scale)
    for k in range(L + 1):
        assert (out[:, k, 0] == N - k).all()  # without NaNs n_k == N - k
        np.testing.assert_array_equal(out[:, k, 1], q[: N - k].sum(axis=0))  # a prefix sum of q
        np.testing.assert_array_equal(out[:, k, 2], q[k:].sum(axis=0))  # a suffix sum
    rows[rng.random(rows.shape) < 0.2] = np.nan
    out = window_autocorr_reference(rows, scale, L, N)
    assert (out[:, 0, 1] == out[:, 0, 2]).all()
    np.testing.assert_array_equal(out[:, 0, 0], np.count_nonzero(~np.isnan(rows[-N:]), axis=0))
    few = window_autocorr_reference(rows[:5], scale, L, 64)
    assert (few[:, 5:] == 0).all() and few[:, 0, 0].max() <= 5  # lags k >= N: all zero


def test_quantisation_rule():
    from rocmdash.ops.window_autocorr import quantise

    x = np.array([0.5, 1.5, 2.5, 3.5, -0.0, -3.0, 4095.0, 4095.49, 4096.0, 1e30, np.inf, -np.inf, np.nan, 0.49999997],
                 np.float32)[:, None]
    q, v = quantise(x, np.ones(1, np.float32))
    assert q[:, 0].tolist() == [0, 2, 2, 4, 0, 0, 4095, 4095, 4095, 4095, 4095, 0, 0, 0]  # half to even
    assert v[:, 0].tolist() == [1] * 12 + [0, 1]
    # the product is one fp32 multiply: 0.1f x 25 is exactly 2.5 in fp32 (2.5000000373 in float64) and rounds to 2
    q, _ = quantise(np.array([[0.1]], np.float32), np.array([25.0], np.float32))
    assert np.float32(0.1) * np.float32(25.0) == np.float32(2.5) and q[0, 0] == 2


# ---- correlogram and period -------------------------------------------------------------
def _sums(x, L, scale=40.95):
    from rocmdash.ops.window_autocorr import window_autocorr_reference

    x = np.asarray(x, np.float32)
    return window_autocorr_reference(x[:, None], np.array([scale], np.float32), L, 1 << 16)[0]


def test_correlogram_edges():
    from rocmdash.ops.window_autocorr import correlogram

    assert np.isnan(correlogram(_sums(np.full(100, 50.0), 8))).all()  # constant
    assert np.isnan(correlogram(_sums(np.full(100, np.nan), 8))).all()  # empty
    assert np.isnan(correlogram(_sums([np.nan] * 50 + [30.0] + [np.nan] * 49, 8))).all()  # n_0 == 1
    assert np.isnan(correlogram(np.zeros((9, 4), np.int64))).all()
    x = np.random.default_rng(0).uniform(0, 100, 100)
    acf = correlogram(_sums(x, 60))
    assert acf[0] == 1.0 and np.isfinite(acf[:51]).all() and np.isnan(acf[51:]).all()  # 2 n_k >= n_0 up to k = 50
    both = correlogram(np.stack([_sums(x, 60), _sums(np.full(100, 1.0), 60)]))
    assert both.shape == (2, 61) and np.isnan(both[1]).all() and (both[0][:51] == acf[:51]).all()
    # Python ints, one division: the largest sums there are do not overflow
    N = 1 << 20
    big = np.array([[N - k, 4095 * (N - k), 4095 * (N - k), 4095 * 4095 * (N - k)] for k in range(3)], np.int64)
    big[0, 3] += 4095  # not constant: var0 > 0
    assert np.isfinite(correlogram(big)).all()


def _square(period, n, sigma, rng, nan=0.01):
    t = np.arange(n)
    x = np.where((t % period) < 0.6 * period, 80.0, 20.0) + rng.normal(0, sigma, n)
    x[rng.random(n) < nan] = np.nan
    return x


@pytest.mark.parametrize("period", [7, 37, 100, 250])
@pytest.mark.parametrize("sigma", [0.0, 15.0])
def test_pick_period_of_noisy_square_waves(period, sigma):
    """60 %-duty square waves over 8192 rows, L = 512, 1 % NaN, noise up to a quarter of the swing."""
    from rocmdash.ops.window_autocorr import correlogram, pick_period

    acf = correlogram(_sums(_square(period, 8192, sigma, np.random.default_rng(period)), 512))
    got, strength = pick_period(acf)
    # the estimator divides a lag's own moments by the lag-0 variance: with NaNs it may pass 1 by a little
    assert got == period and 0.5 <= strength < 1.01 and strength == acf[period]


def test_pick_period_of_a_sine_between_two_lags():
    from rocmdash.ops.window_autocorr import correlogram, pick_period

    x = 50 + 40 * np.sin(2 * np.pi * np.arange(8192) / 64.5)
    got, strength = pick_period(correlogram(_sums(x, 512)))
    assert got in (64, 65) and strength > 0.9


def test_pick_period_returns_nothing_without_rhythm():
    from rocmdash.ops.window_autocorr import correlogram, pick_period

    rng = np.random.default_rng(11)
    noise = rng.uniform(0, 100, 8192)
    walk = 50 + np.cumsum(rng.normal(0, 0.3, 8192))
    for x in (noise, walk, np.full(8192, 42.0)):
        assert pick_period(correlogram(_sums(x, 512))) == (None, None)
    assert pick_period(np.full(20, np.nan)) == (None, None)
    assert pick_period(np.linspace(1.0, 0.1, 20)) == (None, None)  # never down to 0
    # the rule, by hand: k0 = 2, candidates 4 (0.6) and 8 (0.62): the smallest within 0.05 of the largest
    acf = np.array([1.0, 0.2, -0.1, 0.3, 0.6, 0.1, -0.2, 0.4, 0.62, 0.3, 0.1])
    assert pick_period(acf) == (4, 0.6)
    assert pick_period(acf, harmonic_tolerance=0.01) == (8, 0.62)
    assert pick_period(acf, min_strength=0.7) == (None, None)


# ---- options ----------------------------------------------------------------------------
def test_parse_and_check_autocorr():
    from rocmdash.ops import window_autocorr as wa

    assert wa.parse_autocorr("512") == (512, 65536) and wa.parse_autocorr(" 64/4096 ") == (64, 4096)
    assert wa.parse_autocorr((8, 64)) == (8, 64) and wa.parse_autocorr(1024) == (1024, 65536)
    assert wa.check_autocorr(1, 64, 4096) == (1, 64) and wa.check_autocorr(63, 64, 64) == (63, 64)
    for bad in ("", "x", "0", "1025", "8/", "8/63", "8/96", "8/32", "8/2097152", "8/64/2", "-1", "1.5", None, True, (1, 2, 3)):
        with pytest.raises(ValueError):
            wa.parse_autocorr(bad)
    for L, span, window in ((64, 64, 4096), (64, 65536, 64), (100, 128, 64), (0, 64, None), (8, 100, None), (8.5, 64, None)):
        with pytest.raises(ValueError):
            wa.check_autocorr(L, span, window)
    for bad in ([1.0, np.nan], [0.0, 1.0], [-1.0, 1.0], [np.inf, 1.0], [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError):
            wa.check_scale(bad, 2)
    assert wa.check_scale(2.0, 3).tolist() == [2.0, 2.0, 2.0]


def test_constants_mirror_the_header():
    from rocmdash.ops import window_autocorr as wa

    text = "".join(open(os.path.join(ROOT, "csrc", f)).read() for f in ("window_autocorr.h", "window_lag_dev.h", "window_autocorr.hip"))

    def const(name):
        """``constexpr <type> name = 123;`` or ``= 1u << 6;`` - nothing else is understood."""
        m = re.search(rf"constexpr \w+ {name} = (?:(\d+)u?|1u << (\d+));", text)
        assert m, f"{name} is no plain integer constant any more"
        return int(m.group(1)) if m.group(1) else 1 << int(m.group(2))

    want = {"kMaxAutocorrLags": wa.MAX_LAGS, "kMinAutocorrSpan": wa.MIN_SPAN, "kMaxAutocorrSpan": wa.MAX_SPAN,
            "kAutocorrChunk": wa.CHUNK, "kAutocorrQMax": wa.Q_MAX, "kFold": wa.FOLD, "kG": wa.SERIES_GROUP,
            "kLB": wa.LAG_BLOCK}
    assert {k: const(k) for k in want} == want
    assert wa.FOLD * wa.Q_MAX ** 2 < 2 ** 31 and wa.Q_MAX ** 2 * wa.MAX_SPAN < 2 ** 44


# ---- kernel resources -------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_autocorr_kernel_has_no_scratch_and_fits_lds(tmp_path):
    """The recipe of test_kernel_resources.py for window_autocorr.hip."""
    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", "window_autocorr.hip"), "-o", str(tmp_path / "k.o"),
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
    assert any("autocorr_ring_kernel" in k for k in kernels), res.stderr[-2000:]
    for k, r in kernels.items():
        assert r["ScratchSize [bytes/lane]"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] <= LDS_BYTES_PER_CU, (k, r)


# ---- agent without a device -------------------------------------------------------------
def test_cpu_agent_window_autocorr_on_a_recording(native):
    from rocmdash.config import SamplerConfig
    from rocmdash.ops.window_autocorr import window_autocorr_reference
    from rocmdash.runtime.agent import GpuAgent

    agent = GpuAgent(0, source="replay", replay=CAPTURE, cfg=SamplerConfig(window=128, ring_capacity=512), use_gpu=False)
    try:
        assert agent.dws is None
        scale = agent.default_autocorr_scale()
        axis = agent.default_bucket_bounds(1)[:, 0].astype(np.float64)
        assert scale.dtype == np.float32 and (scale == (4095.0 / axis).astype(np.float32)).all()
        empty = agent.window_autocorr(16).numpy()
        assert empty.shape == (len(agent.series), 17, 4) and empty.dtype == np.int64 and (empty == 0).all()
        agent.prefill(150)
        custom = np.full(len(agent.series), 3.0, np.float32)
        for L, span, sc, want_sc in ((16, None, None, scale), (40, 64, None, scale), (16, None, custom, custom)):
            got = agent.window_autocorr(L, span, sc).numpy()
            s = 0
            for i, r in enumerate(agent.rings):
                rows, _ = agent.window_host(i)
                rows = np.asarray(rows, np.float32).reshape(-1, r.width)
                np.testing.assert_array_equal(got[s:s + r.width], window_autocorr_reference(rows, want_sc[s:s + r.width], L, span))
                s += r.width
            assert got[:, 0, 0].max() == min(128, span or 128)
        for kw in (dict(L=0), dict(L=128), dict(L=8, span=100), dict(L=8, scale=np.zeros(len(agent.series), np.float32))):
            with pytest.raises(ValueError):
                agent.window_autocorr(**kw)
    finally:
        agent.close()


# ---- figure -----------------------------------------------------------------------------
def test_create_autocorr_json():
    from rocmdash.viz.figures import create_autocorr

    nan = float("nan")
    fig = create_autocorr("GPU 0: power", [[1.0, 0.25, -0.5, 0.75, nan], [1.0, nan, nan, nan, nan]], ["a", "b"], [3, None])
    doc = json.loads(fig.to_json())
    assert [t["name"] for t in doc["data"]] == ["a", "a period 3", "b"]
    assert doc["data"][0]["x"] == [0, 1, 2, 3, 4] and doc["data"][0]["y"] == [1.0, 0.25, -0.5, 0.75, None]
    assert doc["data"][1]["x"] == [3] and doc["data"][1]["y"] == [0.75] and doc["data"][1]["mode"] == "markers"
    assert doc["layout"]["xaxis"]["title"]["text"] == "lag (samples)" and doc["layout"]["yaxis"]["range"] == [-1, 1]
    assert json.loads(fig.to_plotly().to_json()) == doc
    one = json.loads(create_autocorr("t", [1.0, 0.5]).to_json())
    assert len(one["data"]) == 1 and one["layout"]["showlegend"] is False


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


def test_exporter_serves_autocorr_json_and_404_without(native, monkeypatch):
    """A synthetic source without a GPU: /autocorr is the documented strict JSON with null for
    NaN; off (the default) it is a 404 with a hint and the snapshot carries nothing."""
    import torch

    from rocmdash.ops.window_autocorr import correlogram, pick_period
    from rocmdash.prom.exporter import Exporter

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # agents on the CPU, wherever this runs
    monkeypatch.delenv("ROCMDASH_WINDOW_AUTOCORR", raising=False)
    src = _local_source(window_autocorr="40/64")
    exp = Exporter(src, hostname="n1")
    try:
        agent = src.agents[0]
        assert agent.dws is None and src.autocorr == (40, 64)
        agent.prefill(70)
        exp.serve("127.0.0.1", 0)
        code, ctype, body = _get(exp.port, "/autocorr?x=1")
        assert code == 200 and ctype == "application/json"
        doc = _strict(body)
        assert set(doc) == {"lags", "span", "series", "gpus"}
        assert doc["lags"] == 40 and doc["span"] == 64 and doc["series"] == list(src.series)
        assert list(doc["gpus"]) == [agent.info.gpu_id]
        per = doc["gpus"][agent.info.gpu_id]
        assert list(per) == list(src.series)
        want = agent.window_autocorr(40, 64, src.autocorr_scale).numpy()
        for s, m in enumerate(src.series):
            d = per[m]
            assert set(d) == {"acf", "pairs", "period_samples", "strength"}
            assert d["pairs"] == want[s, :, 0].tolist() and all(isinstance(v, int) for v in d["pairs"])
            acf = correlogram(want[s])
            assert len(d["acf"]) == 41 and d["acf"] == [None if v != v else float(v) for v in acf]
            period, strength = pick_period(acf)
            assert d["period_samples"] == period and d["strength"] == strength
        assert any(v is None for m in per.values() for v in m["acf"])  # lags beyond half the pairs: null
        assert _get(exp.port, "/joint")[0] == 404 and _get(exp.port, "/trend")[0] == 404
    finally:
        exp.close()

    src = _local_source()
    exp = Exporter(src, hostname="n1")
    try:
        assert src.autocorr is None and src.autocorr_scale is None
        exp.serve("127.0.0.1", 0)
        code, _, body = _get(exp.port, "/autocorr")
        assert code == 404 and b"--window-autocorr" in body
        metrics = _get(exp.port, "/metrics")
        assert metrics[0] == 200 and b"rocmdash_window_period" not in metrics[2]
        snap, _ = src.collect()
        assert snap.window_autocorr is None and snap.window_autocorr_span is None
    finally:
        exp.close()


def test_period_gauges_only_where_there_is_a_period():
    """/metrics of a snapshot with sums: the two families for the periodic series only; without
    sums the text is what it was."""
    import copy

    from rocmdash.prom.exporter import SyntheticSource, render_autocorr
    from rocmdash.prom.exposition import render_snapshot

    snap, _ = SyntheticSource(2, seed=3).collect()
    snap.window_series = tuple(snap.columns[:3])
    snap.window = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    off = render_snapshot(snap, hostname="n1")
    assert render_autocorr(snap) is None and "rocmdash_window_period" not in off
    rng = np.random.default_rng(2)
    series = [_square(37, 4096, 5.0, rng), rng.uniform(0, 100, 4096), np.full(4096, 10.0)]
    sums = np.stack([_sums(x, 128) for x in series])
    on = copy.copy(snap)
    on.window_autocorr, on.window_autocorr_span = np.stack([sums, sums[::-1]]), 4096
    text = render_snapshot(on, hostname="n1")
    added = [ln for ln in text.splitlines() if ln not in off.splitlines()]
    assert "\n".join(ln for ln in text.splitlines() if ln not in added) == off.rstrip("\n")
    values = [ln for ln in added if not ln.startswith("#")]
    assert len(values) == 4 and all("rocmdash_window_period_" in ln for ln in values)
    g0, g1 = snap.gpu_ids
    want = {(g0, snap.columns[0]), (g1, snap.columns[2])}
    for fam in ("rocmdash_window_period_samples", "rocmdash_window_period_strength"):
        lines = [ln for ln in values if ln.startswith(fam + "{")]
        assert {(re.search(r'gpu_id="([^"]*)"', ln).group(1), re.search(r'metric="([^"]*)"', ln).group(1)) for ln in lines} == want
    assert all(ln.rsplit(" ", 1)[1] == "37" for ln in values if ln.startswith("rocmdash_window_period_samples"))
    assert all(0.5 <= float(ln.rsplit(" ", 1)[1]) < 1.01 for ln in values if ln.startswith("rocmdash_window_period_strength"))
    doc = _strict(render_autocorr(on))
    assert doc["lags"] == 128 and doc["span"] == 4096
    assert doc["gpus"][g0][snap.columns[0]]["period_samples"] == 37 and doc["gpus"][g0][snap.columns[1]]["period_samples"] is None
    assert doc["gpus"][g0][snap.columns[2]]["acf"] == [None] * 129 and doc["gpus"][g0][snap.columns[2]]["strength"] is None


def test_exporter_option_from_the_environment_and_refusals(native, monkeypatch, capsys):
    import torch

    from rocmdash.prom.exporter import main

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCMDASH_WINDOW_AUTOCORR", "16")
    src = _local_source()
    try:
        assert src.autocorr == (16, 65536)
        src.agents[0].prefill(70)
        snap, _ = src.collect()
        assert snap.window_autocorr.shape == (1, len(src.series), 17, 4) and snap.window_autocorr.dtype == np.int64
        assert snap.window_autocorr_span == 65536 and snap.window_autocorr[0, :, 0, 0].max() == 64
    finally:
        src.close()
    for bad in ("0", "2000", "8/100", "64", "abc"):  # 64 lags need more than the window's 64 rows
        monkeypatch.setenv("ROCMDASH_WINDOW_AUTOCORR", bad)
        with pytest.raises(ValueError):
            _local_source()
    for bad in ("0", "8/100", "x/64"):
        with pytest.raises(SystemExit):
            main(["--window-autocorr", bad])
        assert "--window-autocorr" in capsys.readouterr().err


# ---- page -------------------------------------------------------------------------------
def test_page_autocorr_figures_only_with_sums():
    from rocmdash.prom.exporter import SyntheticSource
    from rocmdash.ui.page import window_autocorr_figures
    from rocmdash.viz.panels import UTIL

    snap, _ = SyntheticSource(2, seed=1).collect()
    assert window_autocorr_figures(snap, snap.gpu_ids) is None  # no sums: the page is as it was
    snap.window_series = (UTIL, "other")
    sums = np.stack([_sums(_square(20, 2048, 3.0, np.random.default_rng(5)), 64), _sums(np.full(2048, 1.0), 64)])
    snap.window_autocorr, snap.window_autocorr_span = np.stack([sums, sums]), 2048
    figs = window_autocorr_figures(snap, [snap.gpu_ids[1]])
    assert [k for k, _ in figs] == [f"plot_autocorr_gpu_util_{snap.gpu_ids[1]}_"]
    doc = json.loads(figs[0][1].to_json())
    assert doc["data"][1]["x"] == [20] and doc["data"][0]["y"][0] == 1.0
