"""The le-bucket kernels (csrc/window_buckets.hip) against the exact integer reference
(rocmdash.ops.window_buckets.window_buckets_reference): one-shot over torch-sorted blocks,
over DeviceWindowSet's resident sorted windows after every refresh of its incremental paths,
over gathered export blocks summed across ranks, and through GpuAgent. Every count must be
EQUAL - on bounds that are sample values (a tie counts as <=) and on bounds one ulp beside
them, between neighbours a few ulp apart - for every family of tests/_exact.py: signed zeros
and denormals, every exponent, tie boundaries, windows of 0..3 valid samples, +-inf."""

import numpy as np
import pytest

import _exact
from _bucket_bounds import bounds_row as _bounds_row
from _bucket_bounds import one_shot_rows as _one_shot_rows
from _window_exports import _assert_counts

pytestmark = pytest.mark.gpu

KINDS = ("on_samples", "between")


def _bounds(x, B, kinds):
    """[S, B] for ``x`` [S, n]; series s takes kinds[s % len(kinds)]."""
    return np.stack([_bounds_row(x[s][~np.isnan(x[s])], B, kinds[s % len(kinds)]) for s in range(len(x))])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [1, 16, 63])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097, 32768])
def test_window_buckets_one_shot(native, cuda, n, B, kind):
    import torch

    from rocmdash.ops.window_buckets import window_buckets

    x = _one_shot_rows(n)
    bounds = _bounds(x, B, (kind,))
    got = window_buckets(torch.from_numpy(np.array(x)).to(cuda), bounds)
    torch.cuda.synchronize()
    want = _assert_counts(got.cpu().numpy(), x, bounds)
    F = _exact.FAMILIES.index
    assert want[F("all_nan")].tolist() == [0] * (B + 1)
    assert want[F("constant"), -1] == n and want[-2, -1] == n
    if kind == "on_samples":
        assert want[F("constant"), 0] == n and want[-2, 0] == n  # a tie on the bound: every sample counts
        if n >= 64 and B > 1:  # B bounds from the smallest finite sample to the largest
            # -inf is in the first bucket, +inf in none but +Inf; -0.0 and +0.0 count under one bound
            assert want[-1, 0] >= 1 and want[-1, B - 1] == n - 1
            z = x[F("zeroes")]
            zb = bounds[F("zeroes")]
            if (zb == 0).any():
                assert want[F("zeroes"), int(np.argmax(zb == 0))] == np.count_nonzero(z <= 0)


def test_window_buckets_rejects_bad_arguments(native, cuda):
    import torch

    from rocmdash.ops.window_buckets import window_buckets

    x = torch.zeros((2, 8), device=cuda)
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [float("inf")], list(range(64))):
        with pytest.raises(ValueError):
            window_buckets(x, bad)
    with pytest.raises(ValueError):
        window_buckets(torch.zeros((2, 0), device=cuda), [1.0])
    with pytest.raises(ValueError):
        window_buckets(torch.zeros((1, 32769), device=cuda), [1.0])
    with pytest.raises(ValueError):
        window_buckets(torch.zeros((2, 8)), [1.0])


class _Mirror:
    """Everything pushed, oldest first."""

    def __init__(self, width):
        self.rows = np.zeros((0, width), np.float32)

    def push(self, x):
        self.rows = np.concatenate([self.rows, x])

    def window(self, W):
        return self.rows[-W:]


def _has_run(seq, run):
    seq = list(seq)
    return any(seq[i:i + len(run)] == list(run) for i in range(len(seq)))


class _Rings:
    """Rings of the given widths in one set, fed consecutive families (wrapping round)."""

    def __init__(self, nat, W, widths):
        self.W, self.widths = W, widths
        self.rings = [nat.SeriesRing(w, 8 * W) for w in widths]
        self.dws = nat.DeviceWindowSet(W, 0)
        for r in self.rings:
            self.dws.add_ring(r)
        self.S = sum(widths)
        self.m = _Mirror(self.S)
        self.rng = np.random.default_rng(W + self.S)
        self.t = 0

    def push(self, k):
        if not k:
            return
        nf = len(_exact.FAMILIES)
        cols = [_exact.family(_exact.FAMILIES[c % nf], self.rng, self.t, k, self.W, blips=(3, self.W + 5))
                for c in range(self.S)]
        x = np.stack(cols, axis=1)
        ts = np.arange(self.t + 1, self.t + 1 + k, dtype=np.uint64)
        c0 = 0
        for r, w in zip(self.rings, self.widths):
            r.push_many(np.ascontiguousarray(x[:, c0:c0 + w]), ts)
            c0 += w
        self.m.push(x)
        self.t += k


@pytest.mark.parametrize("W", [64, 4096])
def test_export_buckets_after_every_refresh(native, cuda, W):
    """Two rings (11 + 5 series) in one DeviceWindowSet, pull mode: a full sort, then the
    incremental paths (one row, none, a few, 255 / 256 rows, a 257-row fall-back) - the
    buckets are exact after EVERY refresh: the half the state names after ``cur`` flips, the
    current ``nvalid``, each ring's series at its offset."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    nat.set_pull_mode(True)
    rs = _Rings(nat, W, (11, 5))
    S, B = rs.S, 16
    out = torch.empty((S, 8), device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    steps = [W + 3, 1, 1, 0, 2, 17, 255, 256, 257, 1]
    rs.push(steps[0])
    # bounds from the first window: on its samples (even series), beside them (odd)
    bounds = _bounds(rs.m.window(W).T, B, KINDS)
    bd = torch.from_numpy(bounds).to(cuda)
    dst = torch.empty((S, B + 1), device=cuda)

    dst.fill_(-1.0)
    rs.dws.export_buckets(bd.data_ptr(), B, dst.data_ptr(), stream)  # no state yet: all zeros
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all()

    blip, blip_nv = _exact.FAMILIES.index("blip"), []
    for i, add in enumerate(steps):
        if i:
            rs.push(add)
        rs.dws.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
        dst.fill_(-1.0)
        rs.dws.export_buckets(bd.data_ptr(), B, dst.data_ptr(), stream)
        torch.cuda.synchronize()
        want = _assert_counts(dst.cpu().numpy(), rs.m.window(W).T, bounds, what=f"after +{add} rows (t = {rs.t})")
        np.testing.assert_array_equal(out.cpu().numpy()[:, 7], want[:, -1])  # +Inf = the stats' count
        blip_nv.append(int(want[blip, -1]))
    assert _has_run(blip_nv, [1, 0]) and _has_run(blip_nv, [0, 1]), blip_nv  # lost every valid sample, got one again
    assert rs.dws.stats()["incremental_launches"] >= 5, rs.dws.stats()


def test_export_buckets_more_series_than_one_launch(native, cuda):
    """9 rings x 15 series = 135 > the 128 series one export_buckets launch holds, B = 63."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    nat.set_pull_mode(True)
    W, B = 64, 63
    rs = _Rings(nat, W, (15,) * 9)
    assert rs.S > int(nat.BUCKET_SERIES_PER_LAUNCH)
    out = torch.empty((rs.S, 8), device=cuda)
    dst = torch.empty((rs.S, B + 1), device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    bd = None
    for add in (W + 3, 1):
        rs.push(add)
        if bd is None:
            bounds = _bounds(rs.m.window(W).T, B, KINDS)
            bd = torch.from_numpy(bounds).to(cuda)
        rs.dws.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
        dst.fill_(-1.0)
        rs.dws.export_buckets(bd.data_ptr(), B, dst.data_ptr(), stream)
        torch.cuda.synchronize()
        _assert_counts(dst.cpu().numpy(), rs.m.window(W).T, bounds, what=f"after +{add} rows")
    for bad_b in (0, 64):
        with pytest.raises(RuntimeError):
            rs.dws.export_buckets(bd.data_ptr(), bad_b, dst.data_ptr(), stream)
    for b_ptr, d_ptr in ((0, dst.data_ptr()), (bd.data_ptr(), 0)):
        with pytest.raises(RuntimeError):
            rs.dws.export_buckets(b_ptr, B, d_ptr, stream)


def _export_blocks(N, S, W, seed):
    """[N, S, 1 + W] export blocks (count, ascending samples, +inf) of N ranks' windows and
    the windows themselves [N, S, W]."""
    x = np.empty((N, S, W), np.float32)
    blocks = np.full((N, S, 1 + W), np.inf, np.float32)
    for i in range(N):
        x[i] = _exact.family_rows(np.random.default_rng(seed + i), 1000 * i, W, W, width=S, blips=(1000 * i + 9,)).T
        for s in range(S):
            v = np.sort(x[i, s][~np.isnan(x[i, s])])
            blocks[i, s, 0] = len(v)
            blocks[i, s, 1:1 + len(v)] = v
    return blocks, x


@pytest.mark.parametrize("N", [1, 2, 8])
def test_bucket_blocks_per_rank_and_node(native, cuda, N):
    import torch

    from rocmdash.ops.window_buckets import window_buckets_reference

    S, W, B = 15, 512, 16
    blocks, x = _export_blocks(N, S, W, seed=N)
    bounds = _bounds(x[0], B, KINDS)  # rank 0's samples: ties there, plain bounds for the others
    want = np.stack([window_buckets_reference(x[i], bounds) for i in range(N)])
    blk = torch.from_numpy(blocks).to(cuda)
    bd = torch.from_numpy(bounds).to(cuda)
    stream = torch.cuda.current_stream().cuda_stream
    per = torch.full((N, S, B + 1), -1.0, device=cuda)
    node = torch.full((S, B + 1), -1.0, device=cuda)
    native.bucket_blocks(blk.data_ptr(), N, S, W, bd.data_ptr(), B, per.data_ptr(), node.data_ptr(), stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(per.cpu().numpy(), want.astype(np.float32))
    np.testing.assert_array_equal(node.cpu().numpy(), want.sum(axis=0).astype(np.float32))
    # either output alone
    per2 = torch.full((N, S, B + 1), -1.0, device=cuda)
    node2 = torch.full((S, B + 1), -1.0, device=cuda)
    native.bucket_blocks(blk.data_ptr(), N, S, W, bd.data_ptr(), B, per2.data_ptr(), 0, stream)
    native.bucket_blocks(blk.data_ptr(), N, S, W, bd.data_ptr(), B, 0, node2.data_ptr(), stream)
    torch.cuda.synchronize()
    assert torch.equal(per2, per) and torch.equal(node2, node)


def test_bucket_blocks_rejects_before_launching(native, cuda):
    import torch

    S, W, B = 3, 16, 4
    blk = torch.zeros((1, S, 1 + W), device=cuda)
    bd = torch.arange(S * B, dtype=torch.float32, device=cuda).reshape(S, B)
    per = torch.full((1, S, B + 1), -1.0, device=cuda)
    node = torch.full((S, B + 1), -1.0, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    args = dict(n=1, w=W, b=B, blocks=blk.data_ptr(), bounds=bd.data_ptr())
    for change in (dict(b=0), dict(b=64), dict(w=0), dict(n=65), dict(blocks=0), dict(bounds=0)):
        a = dict(args, **change)
        with pytest.raises(RuntimeError):
            native.bucket_blocks(a["blocks"], a["n"], S, a["w"], a["bounds"], a["b"], per.data_ptr(), node.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool((per == -1).all()) and bool((node == -1).all())  # nothing ran
    native.bucket_blocks(blk.data_ptr(), 1, S, W, bd.data_ptr(), B, per.data_ptr(), node.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool((per == 0).all()) and bool((node == 0).all())  # count 0: empty windows


def test_agent_window_buckets_end_to_end(native, cuda):
    """GpuAgent on the GPU: window_buckets() in stream order after refresh() equals the
    reference over each ring's host window, and its +Inf bucket the stats' count."""
    import torch

    from rocmdash.config import SamplerConfig
    from rocmdash.ops.window_buckets import window_buckets_reference
    from rocmdash.runtime.agent import GpuAgent

    agent = GpuAgent(0, source="synthetic", counters="synthetic", cfg=SamplerConfig(window=256, ring_capacity=1024))
    try:
        assert agent.dws is not None
        agent.prefill(300)
        for more in (0, 1, 7):  # a full sort, then incremental refreshes
            for _ in range(more):
                agent.sample()
            st = agent.refresh()
            bk = agent.window_buckets()
            torch.cuda.synchronize()
            bounds = agent.default_bucket_bounds()
            got = bk.cpu().numpy()
            assert got.shape == (len(agent.series), 17)
            s = 0
            for i, r in enumerate(agent.rings):
                rows, _ = agent.window_host(i)
                want = window_buckets_reference(rows.T, bounds[s:s + r.width])
                np.testing.assert_array_equal(got[s:s + r.width], want.astype(np.float32))
                s += r.width
            np.testing.assert_array_equal(got[:, -1], st.cpu().numpy()[:, 7])
            assert got[:, -1].max() == 256
        mine = np.linspace(5.0, 95.0, 7, dtype=np.float32)
        a = agent.window_buckets(mine).cpu().numpy()
        b = agent.window_buckets(mine)  # the cached upload and buffer
        torch.cuda.synchronize()
        rows, _ = agent.window_host(0)
        np.testing.assert_array_equal(a[: rows.shape[1]], window_buckets_reference(rows.T, mine).astype(np.float32))
        np.testing.assert_array_equal(b.cpu().numpy(), a)
    finally:
        agent.close()


def test_exporter_serves_bucket_families_and_the_fleet_query(native, cuda):
    """LocalNodeSource with buckets on: /metrics carries both families, cumulative and
    consistent with the window's sample count, and the example histogram_quantile query
    answers through the mini-Prometheus; off (the default), neither family is there."""
    from rocmdash.config import SamplerConfig
    from rocmdash.prom.exporter import Exporter, LocalNodeSource
    from rocmdash.prom.exposition import parse_text
    from rocmdash.prom.mini import MiniPrometheus

    cfg = SamplerConfig(window=64, ring_capacity=256, smi_hz=200, counter_hz=400)
    src = LocalNodeSource(devices=[0], source="synthetic", counters="synthetic", cfg=cfg, window_buckets=8)
    exp = Exporter(src, hostname="n1")
    try:
        src.agents[0].stop()  # the background samplers: the rows below are pushed from this thread
        src.agents[0].prefill(70)
        samples = parse_text(exp.render())
    finally:
        exp.close()
    per = [s for s in samples if s.name == "rocmdash_window_bucket"]
    node = [s for s in samples if s.name == "rocmdash_node_window_bucket"]
    S = len(src.series)
    assert len(per) == S * 9 and len(node) == S * 9
    count = {s.label_dict()["metric"]: s.value for s in samples if s.name == "rocmdash_window_samples"}
    for fam in (per, node):  # one GPU: the node's buckets are its buckets
        for metric in src.series:
            rows = [s for s in fam if s.label_dict()["metric"] == metric]
            assert [s.label_dict()["le"] for s in rows][-1] == "+Inf"
            v = [s.value for s in rows]
            assert v == sorted(v) and v[-1] == count[metric] == 64
    prom = MiniPrometheus()
    prom.db.add_many([(dict(s.label_dict(), __name__=s.name), s.value) for s in samples])
    res = prom.query('histogram_quantile(0.99, sum by (le) (rocmdash_window_bucket{metric="amd_gpu_junction_temperature"}))')
    assert len(res["result"]) == 1 and 0.0 < float(res["result"][0]["value"][1]) <= 110.0

    off = LocalNodeSource(devices=[0], source="synthetic", counters="synthetic", cfg=cfg)
    exp = Exporter(off)
    try:
        assert off.bucket_bounds is None and "_bucket{" not in exp.render().replace("_seconds_bucket{", "")
    finally:
        exp.close()
