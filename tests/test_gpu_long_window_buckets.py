"""The streaming le-bucket kernels (csrc/long_window_buckets.hip) on the GPU: the one-shot
``bucket_ring`` over every window kind of a time-major ring, a ring that takes a full grid of
workgroups, a count past 2^24, ``LongWindowSet.export_buckets`` over a filling and a wrapping
device ring, the argument checks, and ``GpuAgent`` / the exporter with a long window.

Every comparison is exact integer equality with ``window_buckets_reference`` /
``bucket_ring_reference`` (or, for the 2^20-row ring, an int64 count by torch on the device).
Every destination is filled with -1 before the call that writes it."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNT = 7  # the window statistics' count column


def _bounds(cols, B):
    """[cols, B] float32, strictly ascending, 0.0 among them, another spacing per series."""
    step = (0.5 + 0.25 * np.arange(cols, dtype=np.float32))[:, None]
    return np.ascontiguousarray((np.arange(B, dtype=np.float32) - np.float32(B // 2))[None, :] * step)


# what a series holds, by its index in the ring (cyclic): a random mix of everything; only NaN;
# only samples below the first bound; only samples above the last; only samples exactly on
# bounds; only +0.0 / -0.0 (0.0 is a bound); finite samples with -inf / +inf; scattered NaN
ROLES = ("mix", "all_nan", "below", "above", "on_bounds", "zeroes", "inf", "nan")


def _series(rng, role, n, b):
    span = float(b[-1] - b[0]) + 2.0
    x = rng.normal(float(b[len(b) // 2]), span / 3, n).astype(np.float32)
    if role == "all_nan":
        x[:] = np.nan
    elif role == "below":
        x = (b[0] - np.float32(1) - np.abs(x)).astype(np.float32)
    elif role == "above":
        x = (b[-1] + np.float32(1) + np.abs(x)).astype(np.float32)
    elif role == "on_bounds":
        x = rng.choice(b, n).astype(np.float32)
    elif role == "zeroes":
        x = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    elif role == "inf":
        u = rng.random(n)
        x[u < 0.2] = -np.inf
        x[u > 0.8] = np.inf
    elif role == "nan":
        x[rng.random(n) < 0.3] = np.nan
    else:  # mix: runs (the kernel counts runs of one bin) and every special value
        x = np.repeat(x[: (n + 6) // 7], 7)[:n].copy()
        u = rng.random(n)
        x[u < 0.1] = rng.choice(b, int((u < 0.1).sum()))
        x[(u >= 0.1) & (u < 0.15)] = np.nan
        x[(u >= 0.15) & (u < 0.2)] = -0.0
        x[(u >= 0.2) & (u < 0.25)] = 0.0
        x[(u >= 0.25) & (u < 0.28)] = np.inf
        x[(u >= 0.28) & (u < 0.31)] = -np.inf
    return x


def _ring(depth, stride, cols, b, seed):
    """[depth, stride]: every row holds samples (a window that is not full leaves valid rows
    outside it), the columns >= cols hold 0.0 - a bound, so a count that read them shows."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((depth, stride), np.float32)
    for c in range(cols):
        rows[:, c] = _series(rng, ROLES[c % len(ROLES)], depth, b[c])
    return rows


def _windows(depth):
    """(kind, head, n)"""
    part = depth // 2 + 3
    return [("n = 0", depth + 5, 0), ("head = 0", 0, 0), ("n = 1", depth + 7, 1), ("part, unwrapped", part, part),
            ("full, aligned", 2 * depth, depth), ("full, two blocks", 2 * depth + depth // 3 + 1, depth),
            ("head > 2^32", (1 << 32) + 12345, part)]


@pytest.mark.parametrize("B", [1, 2, 16, 63])
@pytest.mark.parametrize("stride,cols", [(1, 1), (3, 3), (8, 5), (12, 12), (16, 16), (64, 64)])
@pytest.mark.parametrize("depth", [1024, 4096, 1 << 17])
def test_bucket_ring_one_shot(native, cuda, depth, stride, cols, B):
    """Every window kind over one ring: empty both ways, one row, part-filled, the whole ring
    as one block and as two, a head past 2^32 (a wrapped part-filled window). 1 and 64 floats
    per row, strides that are no multiple of 4, fewer series than columns; one workgroup
    (1024 x 1) up to 1024 of them (2^17 x 64)."""
    import torch

    from rocmdash.ops.window_buckets import bucket_ring_reference

    b = _bounds(cols, B)
    rows = _ring(depth, stride, cols, b, seed=depth + 64 * stride + B)
    ring = torch.from_numpy(rows).to(cuda)
    bd = torch.from_numpy(b).to(cuda)
    dst = torch.empty((cols + 1, B + 1), dtype=torch.float64, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    for kind, head, n in _windows(depth):
        dst.fill_(-1.0)
        native.bucket_ring(ring.data_ptr(), stride, cols, depth, head, n, bd.data_ptr(), B, dst.data_ptr(), stream)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        want = bucket_ring_reference(rows, head, n, b)
        assert want.shape == (cols, B + 1) and want[:, -1].max() <= n
        np.testing.assert_array_equal(got[:cols], want.astype(np.float64), err_msg=kind)
        assert (got[cols] == -1).all(), f"{kind}: wrote past the last series"
        if n == depth and cols >= 4:  # the roles took effect
            assert want[1, -1] == 0 and (want[2] == n).all() and (want[3, :-1] == 0).all() and want[3, -1] == n


def test_long_window_buckets_op(native, cuda):
    """``long_window_buckets`` with n > 32768: float64 from the streamed ring, equal to the
    reference; at n = 32768 it gives the counts of ``window_buckets``, which keeps the sorted
    path and float32."""
    import torch

    from rocmdash.ops.window_buckets import long_window_buckets, window_buckets, window_buckets_reference

    n = 40000  # a ring of 65536 rows, part-filled
    b = _bounds(5, 16)
    rng = np.random.default_rng(40000)
    x = np.stack([_series(rng, ROLES[c], n, b[c]) for c in range(5)])
    got = long_window_buckets(torch.from_numpy(x).to(cuda), b)
    xs = torch.from_numpy(x[:, :32768].copy()).to(cuda)
    short, same = window_buckets(xs, b), long_window_buckets(xs, b)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and same.dtype == torch.float64 and short.dtype == torch.float32
    np.testing.assert_array_equal(got.cpu().numpy(), window_buckets_reference(x, b).astype(np.float64))
    np.testing.assert_array_equal(short.cpu().numpy(), window_buckets_reference(x[:, :32768], b).astype(np.float32))
    np.testing.assert_array_equal(same.cpu().numpy(), short.cpu().numpy().astype(np.float64))
    with pytest.raises(ValueError):
        long_window_buckets(torch.zeros((65, 8), device=cuda), [1.0])
    with pytest.raises(ValueError):
        long_window_buckets(torch.zeros((2, 8)), [1.0])


def test_bucket_ring_many_workgroups_and_bit_for_bit(native, cuda):
    """2^20 rows x 12 series, B = 16, the whole ring as two blocks: 1024 workgroups adding onto
    the same bins. Exact against an int64 count by torch on the device; two runs into two
    buffers agree bit for bit."""
    import torch

    depth, S, B = 1 << 20, 12, 16
    b = _bounds(S, B)
    g = torch.Generator(device="cpu").manual_seed(20)
    x = torch.randn((depth, S), generator=g) * 3.0
    x[torch.rand((depth, S), generator=g) < 0.05] = float("nan")
    x[::97, 3] = float("inf")
    x[::89, 4] = -0.0
    x = x.to(cuda)
    bd = torch.from_numpy(b).to(cuda)
    stream = torch.cuda.current_stream().cuda_stream
    outs = [torch.full((S, B + 1), -1.0, dtype=torch.float64, device=cuda) for _ in range(2)]
    for o in outs:
        native.bucket_ring(x.data_ptr(), S, S, depth, 3 * depth + 777, depth, bd.data_ptr(), B, o.data_ptr(), stream)
    valid = ~torch.isnan(x)
    want = torch.empty((S, B + 1), dtype=torch.int64, device=cuda)
    for k in range(B):
        want[:, k] = ((x <= bd[:, k]) & valid).sum(dim=0)
    want[:, B] = valid.sum(dim=0)
    torch.cuda.synchronize()
    assert int(want[:, B].min()) > depth // 2
    assert torch.equal(outs[0], want.to(torch.float64))
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))


def test_bucket_ring_counts_past_fp32(native, cuda):
    """2^24 + 3 valid samples below the one bound, in a ring of 2^25 rows (every other row
    holds the same value: a count that read one too many shows): exactly 16777219, which
    float32 cannot hold."""
    import torch

    depth, n = 1 << 25, (1 << 24) + 3
    ring = torch.ones((depth, 1), device=cuda)
    bd = torch.tensor([[2.0]], device=cuda)
    dst = torch.full((1, 2), -1.0, dtype=torch.float64, device=cuda)
    native.bucket_ring(ring.data_ptr(), 1, 1, depth, depth + 5, n, bd.data_ptr(), 1, dst.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert got.dtype == np.float64 and got[0, 0] == 16777219.0 and got[0, 1] == 16777219.0
    assert got[0, 0] != float(np.float32(16777219))


def _push(ring, rng, t, add, width):
    x = rng.normal(0.0, 2.0, (add, width)).astype(np.float32) * (1 + np.arange(width, dtype=np.float32))
    x = np.repeat(x[: (add + 4) // 5], 5, axis=0)[:add].copy()  # runs, as telemetry has
    x[rng.random((add, width)) < 0.04] = np.nan
    x[:, width - 1] = np.nan  # one series without a valid sample
    ring.push_many(x, np.arange(t + 1, t + 1 + add, dtype=np.uint64))
    return x


@pytest.mark.parametrize("W", [1024, 65536])
def test_long_window_export_buckets(native, cuda, W):
    """One ring of 12 series in a LongWindowSet: before any refresh (all zero), a half-filled
    window, a full one, +100 rows, and enough rows to wrap the device ring - exact against a
    host mirror, the last column equal to the refresh's count. Rows pushed after a refresh
    are not in its window: the export still gives the window of that refresh."""
    import torch

    from rocmdash.ops.window_buckets import window_buckets_reference

    nat = native
    nat.set_pinned_host_rings(True)
    B = 16
    ring = nat.SeriesRing(12, 2 * W)
    lw = nat.LongWindowSet(W, 0)
    lw.add_ring(ring)
    b = _bounds(12, B) * np.float32(2.0)
    bd = torch.from_numpy(b).to(cuda)
    out = torch.empty((12, 8), device=cuda)
    dst = torch.empty((13, B + 1), dtype=torch.float64, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    dst.fill_(-1.0)
    lw.export_buckets(bd.data_ptr(), B, dst.data_ptr(), stream)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:12] == 0).all() and (got[12] == -1).all()

    rng = np.random.default_rng(W)
    rows = np.zeros((0, 12), np.float32)
    t = 0
    for add in (W // 2 + 5, W // 2 + 32, 100, W + W // 4 + 7):
        rows = np.concatenate([rows, _push(ring, rng, t, add, 12)])[-W:]
        t += add
        lw.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
        dst.fill_(-1.0)
        lw.export_buckets(bd.data_ptr(), B, dst.data_ptr(), stream)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        want = window_buckets_reference(rows.T, b)
        np.testing.assert_array_equal(got[:12], want.astype(np.float64), err_msg=f"after +{add} rows (t = {t})")
        np.testing.assert_array_equal(got[:12, B], out.cpu().numpy()[:, COUNT].astype(np.float64))
        assert (got[12] == -1).all()
    assert lw.stats()["rows_lost"] == 0 and want[:11, B].min() > 0 and want[11, B] == 0

    _push(ring, rng, t, 9, 12)  # no refresh: the device window is still the one above
    dst.fill_(-1.0)
    lw.export_buckets(bd.data_ptr(), B, dst.data_ptr(), stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy()[:12], want.astype(np.float64))


def test_long_window_export_buckets_two_rings(native, cuda):
    """11 + 5 series in two rings of different fill: the series come in set order, each ring
    over its own window."""
    import torch

    from rocmdash.ops.window_buckets import window_buckets_reference

    nat = native
    nat.set_pinned_host_rings(True)
    W, B = 2048, 7
    rings = [nat.SeriesRing(11, 2 * W), nat.SeriesRing(5, 2 * W)]
    lw = nat.LongWindowSet(W, 0)
    assert [lw.add_ring(r) for r in rings] == [0, 11]
    b = _bounds(16, B) * np.float32(3.0)
    bd = torch.from_numpy(b).to(cuda)
    out = torch.empty((16, 8), device=cuda)
    dst = torch.full((17, B + 1), -1.0, dtype=torch.float64, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(16)
    xa = _push(rings[0], rng, 0, W + 300, 11)[-W:]
    xb = _push(rings[1], rng, 0, 777, 5)
    lw.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
    lw.export_buckets(bd.data_ptr(), B, dst.data_ptr(), stream)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    np.testing.assert_array_equal(got[:11], window_buckets_reference(xa.T, b[:11]).astype(np.float64))
    np.testing.assert_array_equal(got[11:16], window_buckets_reference(xb.T, b[11:]).astype(np.float64))
    np.testing.assert_array_equal(got[:16, B], out.cpu().numpy()[:, COUNT].astype(np.float64))
    assert (got[16] == -1).all()


def test_bucket_entries_reject_before_launching(native, cuda):
    """B outside [1, 63], a null pointer, a depth that is no power of two, n past the depth or
    the head, a stride outside [1, 64] and cols outside [1, stride] raise with nothing
    launched or zeroed: the -1-filled destination is untouched."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    dst = torch.full((66, 65), -1.0, dtype=torch.float64, device=cuda)
    W = 64
    ring_mem = torch.zeros((2 * W, 65), device=cuda)
    bd = torch.from_numpy(_bounds(65, 64)).to(cuda)

    def one_shot(B=8, depth=2 * W, n=W, head=W, d=None, base=None, bounds=None, stride=4, cols=4):
        nat.bucket_ring(ring_mem.data_ptr() if base is None else base, stride, cols, depth, head, n,
                        bd.data_ptr() if bounds is None else bounds, B, dst.data_ptr() if d is None else d, stream)

    bad = [dict(B=0), dict(B=64), dict(base=0), dict(bounds=0), dict(d=0), dict(depth=96), dict(depth=0),
           dict(n=2 * W + 1, head=4 * W), dict(n=W, head=W - 1), dict(stride=0, cols=0), dict(stride=65, cols=65),
           dict(cols=5), dict(cols=0)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            one_shot(**kw)

    rl = nat.SeriesRing(4, 1 << 10)
    lw = nat.LongWindowSet(1 << 10, 0)
    lw.add_ring(rl)
    for args in ((bd.data_ptr(), 0, dst.data_ptr()), (bd.data_ptr(), 64, dst.data_ptr()), (0, 8, dst.data_ptr()),
                 (bd.data_ptr(), 8, 0)):
        with pytest.raises(RuntimeError):
            lw.export_buckets(*args, stream)
    torch.cuda.synchronize()
    assert bool((dst == -1).all())  # nothing ran
    one_shot(n=0, head=0)  # a valid call: every count zero
    torch.cuda.synchronize()
    got = dst.cpu().numpy().reshape(-1)
    assert (got[:4 * 9] == 0).all() and (got[4 * 9:] == -1).all()


def test_agent_window_buckets_with_a_long_window(native, cuda):
    """GpuAgent with cfg.long_window: window_buckets() in stream order after refresh() is
    float64 [S, B + 1], equal to the reference over each ring's host window, its last column
    the refresh's count."""
    import torch

    from rocmdash.config import SamplerConfig
    from rocmdash.ops.window_buckets import bucket_ring_reference, window_buckets_reference
    from rocmdash.runtime.agent import GpuAgent

    W = 1 << 16
    cfg = SamplerConfig(window=W, ring_capacity=W)
    assert cfg.long_window
    agent = GpuAgent(0, source="synthetic", counters="synthetic", cfg=cfg)
    try:
        assert type(agent.dws).__name__ == "LongWindowSet"
        agent.prefill(W + 44)
        bounds = agent.default_bucket_bounds(16)
        for more in (0, 1, 7):
            for _ in range(more):
                agent.sample()
            st = agent.refresh()
            bk = agent.window_buckets(bounds)
            torch.cuda.synchronize()
            got = bk.cpu().numpy()
            assert got.dtype == np.float64 and got.shape == (len(agent.series), 17)
            s = 0
            for i, r in enumerate(agent.rings):
                rows, _ = agent.window_host(i)
                want = window_buckets_reference(np.asarray(rows).T, bounds[s:s + r.width])
                np.testing.assert_array_equal(got[s:s + r.width], want.astype(np.float64), err_msg=f"ring {i}")
                ring = np.zeros((W, r.width), np.float32)  # the same window as a ring at its head
                ring[np.arange(r.head - len(rows), r.head) & (W - 1)] = rows
                np.testing.assert_array_equal(bucket_ring_reference(ring, r.head, len(rows), bounds[s:s + r.width]), want)
                s += r.width
            np.testing.assert_array_equal(got[:, -1], st.cpu().numpy()[:, COUNT].astype(np.float64))
            assert got[:, -1].max() == W
        assert agent.window_buckets(bounds) is bk  # the buffer is reused
    finally:
        agent.close()


def test_exporter_long_window_buckets_in_metrics(native, cuda):
    """LocalNodeSource with a long window and buckets on: /metrics carries both families,
    cumulative, the +Inf bucket equal to the window's sample count."""
    from rocmdash.config import SamplerConfig
    from rocmdash.prom.exporter import Exporter, LocalNodeSource
    from rocmdash.prom.exposition import parse_text

    W = 1 << 16
    cfg = SamplerConfig(window=W, ring_capacity=W, smi_hz=200, counter_hz=400)
    src = LocalNodeSource(devices=[0], source="synthetic", counters="synthetic", cfg=cfg, window_buckets=8)
    exp = Exporter(src, hostname="n1")
    try:
        src.agents[0].stop()  # the background samplers: the rows below are pushed from this thread
        src.agents[0].prefill(W + 70)
        samples = parse_text(exp.render())
        snap = exp._cached[0]
    finally:
        exp.close()
    assert snap.window_buckets.dtype == np.float64 and snap.node_window_buckets.dtype == np.float64
    per = [s for s in samples if s.name == "rocmdash_window_bucket"]
    node = [s for s in samples if s.name == "rocmdash_node_window_bucket"]
    S = len(src.series)
    assert len(per) == S * 9 and len(node) == S * 9
    count = {s.label_dict()["metric"]: s.value for s in samples if s.name == "rocmdash_window_samples"}
    assert max(count.values()) == W
    for fam in (per, node):  # one GPU: the node's buckets are its buckets
        for metric in src.series:
            vals = [s.value for s in fam if s.label_dict()["metric"] == metric]
            assert len(vals) == 9 and vals == sorted(vals) and vals[-1] == count[metric], (metric, vals)
