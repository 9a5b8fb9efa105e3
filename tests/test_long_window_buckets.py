"""Long-window le-buckets without a GPU: the ring reference against brute force, the
exporter's node sum and the exposition's integers past 2^24, and the streaming kernels'
resources (csrc/long_window_buckets.hip, cross-compiled for gfx950)."""

import os
import re
import subprocess

import numpy as np
import pytest

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
