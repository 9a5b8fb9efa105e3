"""Long-window le-buckets without a GPU: the ring reference against brute force, the
exporter's node sum and the exposition's integers past 2^24, and the streaming kernels'
resources (csrc/long_window_buckets.hip, cross-compiled for gfx950)."""

import os
import re
import subprocess

import numpy as np
import pytest

import _bucket_bounds as bb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _brute(rows, head, n, bounds):
    """Row by row, sample by sample, in Python: int64 [cols, B + 1]."""
    depth = rows.shape[0]
    out = np.zeros((bounds.shape[0], bounds.shape[1] + 1), np.int64)
    for r in range(head - n, head):
        for c in range(bounds.shape[0]):
            x = rows[r % depth, c]
            if x != x:
                continue
            out[c, -1] += 1
            for k in range(bounds.shape[1]):
                out[c, k] += bool(x <= bounds[c, k])
    return out


@pytest.mark.parametrize("depth,stride,cols,head,n", [
    (8, 1, 1, 0, 0), (8, 3, 3, 5, 5), (8, 3, 2, 8, 8), (16, 4, 3, 21, 16), (16, 4, 4, 27, 9), (32, 5, 5, 100, 1),
    (64, 2, 2, (1 << 32) + 7, 40), (64, 2, 1, 70, 0)])
def test_bucket_ring_reference_against_brute_force(depth, stride, cols, head, n):
    from rocmdash.ops.window_buckets import bucket_ring_reference

    rng = np.random.default_rng(depth + head % 1000 + n)
    bounds = np.sort(rng.normal(0, 1, (cols, 4)).astype(np.float32), axis=1)
    bounds[:, 1] = 0.0 if (bounds[:, 0] < 0).all() and (bounds[:, 2] > 0).all() else bounds[:, 1]
    rows = rng.normal(0, 1, (depth, stride)).astype(np.float32)
    rows[rng.random(rows.shape) < 0.2] = np.nan
    rows[rng.random(rows.shape) < 0.1] = -0.0
    rows[rng.random(rows.shape) < 0.1] = 0.0
    rows[rng.random(rows.shape) < 0.05] = np.inf
    rows[rng.random(rows.shape) < 0.05] = -np.inf
    rows[0, 0] = bounds[0, 2]  # a tie
    got = bucket_ring_reference(rows, head, n, bounds)
    assert got.dtype == np.int64 and got.shape == (cols, 5)
    np.testing.assert_array_equal(got, _brute(rows, head, n, bounds))
    if cols == stride:  # [B]: the same bounds for every column
        np.testing.assert_array_equal(bucket_ring_reference(rows, head, n, bounds[0]),
                                      _brute(rows, head, n, np.tile(bounds[0], (cols, 1))))


@pytest.mark.parametrize("B", [1, 2, 3, 16, 63])
@pytest.mark.parametrize("name", bb.BOUNDS)
def test_bounds_families_are_bounds_and_the_reference_counts_them(name, B):
    """Every family of tests/_bucket_bounds.py is finite and strictly ascending at every B
    the GPU tests use, and ``bucket_ring_reference`` on it - every sample family in one ring,
    a wrapped window - is the brute-force ``x <= b`` count."""
    from rocmdash.ops.window_buckets import bucket_ring_reference, check_bounds

    depth, head, n = 64, (1 << 32) + 37, 50
    rng = np.random.default_rng(B + len(name))
    cols = [bb.column(rng, name, kind, 2 + j, depth, B) for j, kind in enumerate(bb.SAMPLE_KINDS)]
    bounds = np.stack([b for b, _ in cols])
    assert bounds.dtype == np.float32 and bounds.shape == (len(cols), B)
    np.testing.assert_array_equal(check_bounds(bounds), bounds)
    rows = np.stack([x for _, x in cols] + [np.full(depth, 1.0, np.float32)], axis=1)  # + an unread column
    assert rows.dtype == np.float32
    got = bucket_ring_reference(rows, head, n, bounds)
    np.testing.assert_array_equal(got, _brute(rows, head, n, bounds))
    assert got[:, -1].max() == n


def _even_bounds(cols, B):
    """``_bounds`` of tests/test_gpu_long_window_buckets.py: what every streaming test used."""
    step = (0.5 + 0.25 * np.arange(cols, dtype=np.float32))[:, None]
    return np.ascontiguousarray((np.arange(B, dtype=np.float32) - np.float32(B // 2))[None, :] * step)


@pytest.mark.parametrize("B", [16, 63])
def test_uneven_bounds_need_the_walk_and_even_ones_do_not(B):
    """The fp32 model of the kernel's guess on ``hop`` samples: the uneven families are far
    off it - geometric bounds at least B / 4 bins below the sample's bin (the walk goes up),
    their mirror image as far above (down), a span that overflows B - 1 bins up from bin 0,
    denormal and clustered bounds B / 4 bins one way or the other - while on the evenly
    spaced bounds of tests/test_gpu_long_window_buckets.py no sample of any family is more
    than ONE bin from its guess: those tests never drove the walk."""
    rng = np.random.default_rng(B)
    reached = {}
    for name in bb.WALKS:
        b = bb.bounds_for(name, B)
        x = bb.hop(rng, 1024, b)
        assert (np.diff(np.searchsorted(b, x, "left")) != 0).all(), f"{name}: a hop sample stayed in its bin"
        reached[name] = bb.walk_reached(x, b)
        assert bb.walks_enough(name, x, b), (name, reached[name])
    print(f"[walk] B = {B}: (up, down) {reached}")
    assert reached["geometric"][0] >= B // 4 and reached["geometric_down"][1] >= B // 4
    assert reached["huge_span"][0] >= B - 1
    assert max(reached["denormal"]) >= B // 4 and max(reached["clustered"]) >= B // 4
    even = _even_bounds(8, B)
    for c in range(8):
        for kind in bb.SAMPLE_KINDS:
            x = bb.exact_column(rng, c, 4096) if kind == "exact" else bb.SAMPLES[kind](rng, 4096, even[c])
            assert max(bb.walk_reached(x, even[c])) <= 1, (c, kind)
        wide = (rng.normal(0, 1, 4096) * float(even[c, -1])).astype(np.float32)  # the ROLES' normal samples
        assert max(bb.walk_reached(wide, even[c])) <= 1, c


def test_guess_distance_is_the_kernels_clamp():
    """NaN -> 0 (inf x 0, 0 x inf), -inf -> 0, +inf -> B; a NaN sample takes no walk."""
    b = bb.huge_span(16)
    x = np.array([-np.inf, np.inf, np.nan, b[0], b[-1]], np.float32)
    np.testing.assert_array_equal(bb.guess_distance(x, b), [0, 16, 0, 0, 15])  # every guess is bin 0
    b = bb.denormal(16)  # bins per unit is inf: b[0] -> 0 x inf = NaN -> 0, all above it -> B
    x = np.array([-np.inf, np.inf, b[0], b[1], b[-1], 1.0], np.float32)
    np.testing.assert_array_equal(bb.guess_distance(x, b), [0, 0, 0, 1 - 16, 15 - 16, 0])
    np.testing.assert_array_equal(bb.guess_distance(np.array([0.5], np.float32), np.array([1.0], np.float32)), [0])


def test_bucket_ring_reference_rejects_bad_rings():
    from rocmdash.ops.window_buckets import bucket_ring_reference

    rows = np.zeros((8, 2), np.float32)
    for kw in (dict(head=4, n=5), dict(head=20, n=9), dict(head=4, n=-1)):
        with pytest.raises(ValueError):
            bucket_ring_reference(rows, bounds=[1.0], **kw)
    with pytest.raises(ValueError):
        bucket_ring_reference(np.zeros((6, 2), np.float32), 4, 4, [1.0])  # depth 6
    with pytest.raises(ValueError):
        bucket_ring_reference(rows, 4, 4, np.ones((3, 1), np.float32))  # 3 series in 2 columns


def test_node_bucket_sum_keeps_the_dtype_and_stays_exact():
    from rocmdash.prom.exporter import node_bucket_sum

    per = np.zeros((8, 2, 3), np.float64)
    per[:, 0, :] = [1.0, (1 << 24) + 1, (1 << 26)]  # 8 x (2^24 + 1): not a float32, nor is any partial sum
    per[:, 1, :] = [0.0, 3.0, (1 << 26) - 1]
    node = node_bucket_sum(per)
    assert node.dtype == np.float64
    np.testing.assert_array_equal(node, [[8.0, (1 << 27) + 8, 1 << 29], [0.0, 24.0, (1 << 29) - 8]])
    assert float(np.float32(node[0, 1])) != node[0, 1] and float(np.float32(node[1, 2])) != node[1, 2]
    short = np.full((64, 2, 3), 32768.0, np.float32)  # the short windows' counts: float32 in, float32 out
    short[:, 1, 0] = 3.0
    node = node_bucket_sum(short)
    assert node.dtype == np.float32
    np.testing.assert_array_equal(node, short.sum(axis=0, dtype=np.float64).astype(np.float32))
    assert node[0, 0] == 64 * 32768 and node[1, 0] == 192


def test_exposition_prints_large_counts_exactly():
    from rocmdash.prom.exposition import Exposition, parse_text

    exp = Exposition()
    vals = [np.float64(16777217), np.float64((1 << 29) + 1), np.array([(1 << 26) + 1], np.float64)[0], 16777219.0]
    for i, v in enumerate(vals):
        exp.add("rocmdash_window_bucket", v, {"le": str(i)}, "h")
    text = exp.text()
    assert 'rocmdash_window_bucket{le="0"} 16777217\n' in text
    assert 'rocmdash_window_bucket{le="1"} 536870913\n' in text
    assert 'rocmdash_window_bucket{le="2"} 67108865\n' in text
    assert [s.value for s in parse_text(text)] == [16777217.0, 536870913.0, 67108865.0, 16777219.0]


def test_snapshot_with_float64_buckets_renders_them_exactly():
    """The counts of a long window through render_snapshot: per GPU and node-wide."""
    from rocmdash.prom.exporter import node_bucket_sum
    from rocmdash.prom.exposition import parse_text, render_snapshot
    from rocmdash.viz.panels import NodeSnapshot

    snap = NodeSnapshot(gpu_ids=["0", "1"], card_models=["m", "m"], columns=("amd_gpu_gfx_activity",),
                        values=np.zeros((2, 1), np.float32))
    snap.window_series = ("amd_gpu_gfx_activity",)
    snap.window_bucket_bounds = np.array([[50.0, 100.0]], np.float32)
    snap.window_buckets = np.array([[[3.0, 16777217.0, 67108864.0]], [[4.0, 16777218.0, 67108863.0]]])
    snap.node_window_buckets = node_bucket_sum(snap.window_buckets)
    samples = parse_text(render_snapshot(snap))
    per = [s.value for s in samples if s.name == "rocmdash_window_bucket"]
    node = [s.value for s in samples if s.name == "rocmdash_node_window_bucket"]
    assert per == [3.0, 16777217.0, 67108864.0, 4.0, 16777218.0, 67108863.0]
    assert node == [7.0, 33554435.0, 134217727.0]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_long_window_buckets_kernels_have_no_scratch(tmp_path):
    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", "long_window_buckets.hip"), "-o", str(tmp_path / "k.o"),
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
        m = re.search(r"(ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name is not None:
            kernels[name][m.group(1)] = int(m.group(2))
    assert any("bucket_ring_kernel" in k for k in kernels) and any("bucket_finalize_kernel" in k for k in kernels)
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", -1) == 0, (k, r)


def test_agent_window_buckets_with_a_long_window_on_the_cpu(native):
    """Without a GPU the agent counts on the host: float64 for a long window, as on the device."""
    from rocmdash.config import SamplerConfig
    from rocmdash.ops.window_buckets import window_buckets_reference
    from rocmdash.runtime.agent import GpuAgent

    W = 1 << 16
    agent = GpuAgent(0, source="synthetic", counters="synthetic", cfg=SamplerConfig(window=W, ring_capacity=W),
                     use_gpu=False)
    try:
        agent.prefill(300)
        got = agent.window_buckets(agent.default_bucket_bounds(4)).numpy()
        assert got.dtype == np.float64 and got.shape == (len(agent.series), 5)
        rows, _ = agent.window_host(0)
        w = agent.rings[0].width
        np.testing.assert_array_equal(got[:w], window_buckets_reference(np.asarray(rows).T, agent.default_bucket_bounds(4)[:w]))
    finally:
        agent.close()
