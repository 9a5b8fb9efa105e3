"""The window-heatmap kernels (csrc/window_heatmap.hip) against the numpy reference of
rocmdash.ops.window_heatmap (itself checked against a per-row loop in test_window_heatmap.py):
the one-shot op over a wrapped ring, DeviceWindowSet.export_heatmap after every refresh of its
incremental paths, LongWindowSet.export_heatmap over a filling, a full and a wrapped device
ring, the argument checks, and GpuAgent end to end.

Counts are integers: every comparison is exact equality. Every buffer is filled with -1 before
the call that writes it, so a (series, slot, bin) the kernel left out shows."""

import numpy as np
import pytest

import _exact
from _window_exports import _assert_heatmap

pytestmark = pytest.mark.gpu

PCT = (50.0, 90.0, 99.0)


def _even_bounds(x, B):
    """[S, B]: per series B evenly spaced bounds over its finite samples' range."""
    out = np.empty((len(x), B), np.float32)
    for s, v in enumerate(x):
        v = v[np.isfinite(v)].astype(np.float64)
        lo, hi = (v.min(), v.max()) if v.size else (0.0, 0.0)
        b = (np.linspace(lo, hi, B) if B > 1 else np.array([(lo + hi) / 2])).astype(np.float32)
        if not (np.isfinite(b).all() and (np.diff(b) > 0).all()):  # one value, or steps below an ulp
            b = (np.float32(lo) + np.arange(B, dtype=np.float32) - np.float32(B // 2)).astype(np.float32)
        if not (np.isfinite(b).all() and (np.diff(b) > 0).all()):
            b = np.arange(B, dtype=np.float32) - np.float32(B // 2)
        out[s] = b
    return out


def _quantile_bounds(x, B):
    """[S, B]: per series B of its own distinct finite samples at evenly spaced ranks - unevenly
    spaced bounds with samples exactly on every one of them (a series with fewer than B distinct
    values: evenly spaced)."""
    out = _even_bounds(x, B)
    for s, v in enumerate(x):
        u = np.unique(v[np.isfinite(v)])
        if len(u) >= B:
            out[s] = u[np.round(np.linspace(0, len(u) - 1, B)).astype(np.int64)]
    return out


_ROWS = {}


def _one_shot_rows(n):
    """[S, n]: the 21 families, + a constant run, + one series with -inf and +inf at its ends."""
    if n not in _ROWS:
        rng = np.random.default_rng(n + 5)
        x = _exact.family_rows(rng, 0, n, n, width=len(_exact.FAMILIES), blips=(n // 2,)).T
        ends = rng.normal(0, 1, n).astype(np.float32)
        ends[0], ends[-1] = -np.inf, np.inf  # n = 1: the one sample is +inf
        x = np.concatenate([x, np.full((1, n), -7.25, np.float32), ends[None]])
        x.setflags(write=False)
        _ROWS[n] = x
    return _ROWS[n]


# series taken per ring stride: 16 = the first families (zeroes, ties, ramps, sparse, inf), 5 =
# wide .. ties, 1 = the +-inf ends
_SLICES = {1: slice(22, 23), 5: slice(2, 7), 16: slice(0, 16), 23: slice(0, 23)}
SHAPES = [(1, 64, 8), (63, 64, 64), (64, 64, 64), (65, 128, 8), (4096, 4096, 64), (4096, 4096, 1024)]
HEADS = ["n", "n+1", "wrapped"]
STRIDES = [1, 5, 16, 23]
BUCKETS = [1, 16, 63]
# The cross product thinned: every (shape, head kind, stride) runs once, with the B and the
# kind of bounds rotating - over the file each stride meets each B with both kinds of bounds.
ONE_SHOT = [(n, W, P, HEADS[h], STRIDES[s], BUCKETS[(i + h + s) % 3], "even" if (i + h) // 3 % 2 == 0 else "quantile")
            for i, (n, W, P) in enumerate(SHAPES) for h in range(3) for s in range(4)]


def test_one_shot_cases_cover_the_cross():
    for stride in STRIDES:
        for B in BUCKETS:
            kinds = {c[6] for c in ONE_SHOT if c[4] == stride and c[5] == B}
            assert kinds == {"even", "quantile"}, (stride, B, kinds)


@pytest.mark.parametrize("n,window,P,head_kind,stride,B,kind", ONE_SHOT)
def test_window_heatmap_one_shot(native, cuda, n, window, P, head_kind, stride, B, kind):
    """The smallest shapes that reach c = 1, a partial first and last slot, the ring wrap, a
    row stride that is no multiple of 4, more slots than rows, and both kernels (a wave or a
    workgroup per slot)."""
    import torch

    from rocmdash.ops.window_buckets import check_bounds
    from rocmdash.ops.window_heatmap import window_heatmap

    head = {"n": n, "n+1": n + 1, "wrapped": 3 * window - 1}[head_kind]
    x = np.array(_one_shot_rows(n)[_SLICES[stride]])  # a writable copy of the shared rows
    assert x.shape == (stride, n)
    bounds = check_bounds((_even_bounds if kind == "even" else _quantile_bounds)(x, B), stride)
    got = window_heatmap(torch.from_numpy(x).to(cuda), P, bounds, head=head, window=window)
    torch.cuda.synchronize()
    want = _assert_heatmap(got.cpu().numpy(), x.T, head, window, P, bounds)
    full = np.count_nonzero(want.sum(axis=(0, 2)))
    assert full <= len({r // (window // P) for r in range(head - n, head)})
    assert want.sum() == np.count_nonzero(~np.isnan(x))


def test_window_heatmap_one_workgroup_streams_many_rows(native, cuda):
    """window 2^17, P = 8: 16384 rows x 3 series per workgroup, far more rows than threads; the
    same bits on a second run."""
    import torch

    from rocmdash.ops.window_heatmap import window_heatmap

    W, P, B = 1 << 17, 8, 16
    rng = np.random.default_rng(17)
    x = np.stack([_exact.family(f, rng, 0, W, W) for f in ("normal_nan", "wide", "zeroes")])
    bounds = _quantile_bounds(x, B)
    head = W + 12345
    xd = torch.from_numpy(x).to(cuda)
    got = window_heatmap(xd, P, bounds, head=head, window=W)
    again = window_heatmap(xd, P, bounds, head=head, window=W)
    torch.cuda.synchronize()
    want = _assert_heatmap(got.cpu().numpy(), x.T, head, W, P, bounds)
    assert (want.sum(axis=2) > 0).all() and want.max() <= 65536
    np.testing.assert_array_equal(again.cpu().numpy(), want)


class _Rings:
    """Rings of the given widths in one DeviceWindowSet, fed consecutive families."""

    def __init__(self, nat, W, widths):
        self.W, self.widths = W, widths
        self.rings = [nat.SeriesRing(w, 8 * W) for w in widths]
        self.dws = nat.DeviceWindowSet(W, 0)
        for r in self.rings:
            self.dws.add_ring(r)
        self.S = sum(widths)
        self.rows = np.zeros((0, self.S), np.float32)  # everything pushed, oldest first
        self.rng = np.random.default_rng(W + self.S + 1)
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
        self.rows = np.concatenate([self.rows, x])
        self.t += k

    def window(self):
        return self.rows[-self.W:] if self.t else self.rows


def _mixed_bounds(rng, S, B):
    """[S, B] unevenly spaced: random levels and the values the tie families sit on."""
    ties = np.array([0, 1, 2, 3, 4, 5, 16, 17, 42, 100], np.float32)
    out = np.empty((S, B), np.float32)
    for s in range(S):
        cand = np.unique(np.concatenate([rng.normal(50, 60, 3 * B).astype(np.float32), ties]))
        out[s] = np.sort(rng.choice(cand, B, replace=False))
    return out


@pytest.mark.parametrize("W,P", [(64, 8), (4096, 64)])
def test_export_heatmap_after_every_refresh(native, cuda, W, P):
    """Two rings (11 + 5 series) in one DeviceWindowSet, pull mode: the heatmap equals the
    reference after EVERY refresh - a full sort, then one row, none, a few, 255 / 256 / 257 -
    each ring's series at its offset; its bins sum to export_trend's counts and its slots,
    summed and cumulated, are export_buckets' counts of the same refresh; a full column keeps its
    bits while the window slides; all zeroes without state."""
    import torch

    from rocmdash.ops.window_trend import trend_geometry

    nat = native
    nat.set_pinned_host_rings(True)
    nat.set_pull_mode(True)
    rs = _Rings(nat, W, (11, 5))
    S, c, B = rs.S, W // P, 16
    bounds = _mixed_bounds(np.random.default_rng(W), S, B)
    bd = torch.from_numpy(bounds).to(cuda)
    out = torch.empty((S, 8), device=cuda)
    dst = torch.empty((S, P + 1, B + 1), dtype=torch.int32, device=cuda)
    trend = torch.empty((S, P + 1, 4), device=cuda)
    buckets = torch.empty((S, B + 1), device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    steps = [W + 3, 1, 1, 0, 2, 17, 255, 256, 257, 1]

    dst.fill_(-1)
    rs.dws.export_heatmap(P, bd.data_ptr(), B, dst.data_ptr(), stream)  # no refresh yet
    torch.cuda.synchronize()
    assert bool((dst == 0).all())

    prev, stable = None, 0
    for add in steps:
        rs.push(add)
        rs.dws.refresh(out.data_ptr(), stream, *PCT)
        dst.fill_(-1)
        trend.fill_(-1.0)
        buckets.fill_(-1.0)
        rs.dws.export_heatmap(P, bd.data_ptr(), B, dst.data_ptr(), stream)
        rs.dws.export_trend(P, trend.data_ptr(), stream)
        rs.dws.export_buckets(bd.data_ptr(), B, buckets.data_ptr(), stream)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        win = rs.window()
        _assert_heatmap(got, win, rs.t, W, P, bounds, what=f"after +{add} rows")
        np.testing.assert_array_equal(got.sum(axis=2), trend.cpu().numpy()[:, :, 3])
        np.testing.assert_array_equal(np.cumsum(got.sum(axis=1), axis=1), buckets.cpu().numpy())
        # a column that is full in both refreshes keeps its bits
        _, ranges = trend_geometry(rs.t, len(win), W, P)
        last = (rs.t - 1) // c
        if prev is not None and add < c:
            plast, pranges, pgot = prev
            for j, (b, e) in enumerate(ranges):
                jp = j + (last - plast)
                if e - b == c and 0 <= jp <= P and pranges[jp, 1] - pranges[jp, 0] == c:
                    assert (pranges[jp] == (b, e)).all()
                    np.testing.assert_array_equal(got[:, j], pgot[:, jp], err_msg=f"column [{b}, {e})")
                    stable += 1
        prev = (last, ranges, got)
    assert stable >= P  # columns were compared

    rs.dws.invalidate()
    dst.fill_(-1)
    rs.dws.export_heatmap(P, bd.data_ptr(), B, dst.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool((dst == 0).all())


@pytest.mark.parametrize("W", [1024, 65536])
def test_long_window_export_heatmap(native, cuda, W):
    """One ring of 12 series in a LongWindowSet, P = 8 (a wave per slot at W = 1024, a
    workgroup at 65536): all zeroes before any refresh; after the first fill (a window that is
    not full yet, then full), after +100 rows, and after enough rows to wrap the device ring the
    heatmap equals the reference over a host mirror, and its slots summed and cumulated are the
    long buckets' float64 counts."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    P, B = 8, 16
    ring = nat.SeriesRing(12, 2 * W)
    lw = nat.LongWindowSet(W, 0)
    lw.add_ring(ring)
    rng = np.random.default_rng(W + P)
    bounds = _mixed_bounds(rng, 12, B)
    bd = torch.from_numpy(bounds).to(cuda)
    out = torch.empty((12, 8), device=cuda)
    dst = torch.empty((12, P + 1, B + 1), dtype=torch.int32, device=cuda)
    buckets = torch.empty((12, B + 1), dtype=torch.float64, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    dst.fill_(-1)
    lw.export_heatmap(P, bd.data_ptr(), B, dst.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool((dst == 0).all())

    rows = np.zeros((0, 12), np.float32)
    t = 0
    for add in (W // 2 + 5, W // 2 + 32, 100, W + W // 4 + 7):
        x = _exact.family_rows(rng, t, add, W, width=12, first=1, blips=(t + 9,))
        ring.push_many(x, np.arange(t + 1, t + 1 + add, dtype=np.uint64))
        rows = np.concatenate([rows, x])[-W:]
        t += add
        lw.refresh(out.data_ptr(), stream, *PCT)
        dst.fill_(-1)
        buckets.fill_(-1.0)
        lw.export_heatmap(P, bd.data_ptr(), B, dst.data_ptr(), stream)
        lw.export_buckets(bd.data_ptr(), B, buckets.data_ptr(), stream)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        _assert_heatmap(got, rows, t, W, P, bounds, what=f"after +{add} rows (t = {t})")
        np.testing.assert_array_equal(np.cumsum(got.sum(axis=1), axis=1).astype(np.float64), buckets.cpu().numpy())
        np.testing.assert_array_equal(got.sum(axis=(1, 2)), out.cpu().numpy()[:, _exact.COUNT])
    assert lw.stats()["rows_lost"] == 0


def test_heatmap_entries_reject_before_launching(native, cuda):
    """The trend's bad cases, B = 0 and B = 64, null bounds and a null or misaligned dst raise
    with nothing launched or written: the -1-filled buffer is untouched."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    dst = torch.full((4 * 2049 * 64,), -1, dtype=torch.int32, device=cuda)
    W = 64
    ring_mem = torch.zeros((2 * W, 4), device=cuda)
    bd = torch.arange(4 * 64, dtype=torch.float32, device=cuda)  # ascending for any B

    def one_shot(P=8, c=None, depth=2 * W, n=W, head=W, d=None, base=None, stride=4, cols=4, B=16, b=None):
        nat.heatmap_ring(ring_mem.data_ptr() if base is None else base, stride, cols, depth, head, n, P,
                         W // P if c is None and P else (c or 0), bd.data_ptr() if b is None else b, B,
                         dst.data_ptr() if d is None else d, stream)

    bad = [dict(P=0), dict(P=6), dict(P=2048), dict(P=128),  # 128 > W: no row per column
           dict(P=8, c=1 << 17, depth=1 << 20),  # W / P > 65536
           dict(c=3), dict(n=2 * W + 1, head=4 * W), dict(n=W, head=W - 1), dict(c=4, n=W), dict(d=0), dict(base=0),
           dict(stride=0), dict(stride=65, cols=65), dict(cols=5), dict(cols=0), dict(depth=96),
           dict(B=0), dict(B=64), dict(b=0), dict(d=dst.data_ptr() + 2), dict(d=dst.data_ptr() + 1)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            one_shot(**kw)

    rd = nat.SeriesRing(4, 8 * W)
    dws = nat.DeviceWindowSet(W, 0)
    dws.add_ring(rd)
    rl = nat.SeriesRing(4, 1 << 10)
    lw = nat.LongWindowSet(1 << 10, 0)
    lw.add_ring(rl)
    big = nat.LongWindowSet(1 << 24, 0)  # no ring: nothing allocated; 2^24 / 128 > 65536
    for ws, too_many in ((dws, 128), (lw, 2048)):
        for P in (0, 6, 2048, too_many):
            with pytest.raises(RuntimeError):
                ws.export_heatmap(P, bd.data_ptr(), 16, dst.data_ptr(), stream)
        for b, B, d in ((bd.data_ptr(), 0, dst.data_ptr()), (bd.data_ptr(), 64, dst.data_ptr()), (0, 16, dst.data_ptr()),
                        (bd.data_ptr(), 16, 0), (bd.data_ptr(), 16, dst.data_ptr() + 2)):
            with pytest.raises(RuntimeError):
                ws.export_heatmap(8, b, B, d, stream)
    with pytest.raises(RuntimeError):
        big.export_heatmap(128, bd.data_ptr(), 16, dst.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool((dst == -1).all())  # nothing ran
    one_shot(n=0, head=0)  # a valid call: every count zero
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:4 * 9 * 17] == 0).all() and (got[4 * 9 * 17:] == -1).all()


@pytest.mark.parametrize("long", [False, True])
def test_agent_window_heatmap_end_to_end(native, cuda, long):
    """GpuAgent on the GPU, short and long window sets: window_heatmap() in stream order after
    refresh() equals the reference over each ring's host window and adds up to its counts; the
    buffer is reused for the same columns and bounds."""
    import torch

    from rocmdash.config import SamplerConfig
    from rocmdash.runtime.agent import GpuAgent

    W = 1 << 16 if long else 256
    cfg = SamplerConfig(window=W, ring_capacity=W if long else 1024)
    agent = GpuAgent(0, source="synthetic", counters="synthetic", cfg=cfg)
    try:
        assert type(agent.dws).__name__ == ("LongWindowSet" if long else "DeviceWindowSet")
        agent.prefill(W + 44 if long else 300)
        bounds = agent.default_bucket_bounds(16)
        for more in (0, 1, 7):
            for _ in range(more):
                agent.sample()
            st = agent.refresh()
            hm = agent.window_heatmap(8)
            torch.cuda.synchronize()
            got = hm.cpu().numpy()
            assert got.shape == (len(agent.series), 9, 17) and got.dtype == np.int32
            s = 0
            for i, r in enumerate(agent.rings):
                rows, _ = agent.window_host(i)
                _assert_heatmap(got[s:s + r.width], rows, r.head, W, 8, bounds[s:s + r.width], what=f"ring {i}")
                s += r.width
            np.testing.assert_array_equal(got.sum(axis=(1, 2)), st.cpu().numpy()[:, 7])
            assert got.sum(axis=(1, 2)).max() == W
        assert agent.window_heatmap(8) is hm  # the buffer is reused
        custom = np.ascontiguousarray(bounds[:, ::3])
        other = agent.window_heatmap(8, custom)
        torch.cuda.synchronize()
        assert other is not hm and other.shape == (len(agent.series), 9, custom.shape[1] + 1)
        assert agent.window_heatmap(8, custom) is other
        np.testing.assert_array_equal(other.cpu().numpy().sum(axis=2), got.sum(axis=2))
        with pytest.raises(ValueError):
            agent.window_heatmap(6)
    finally:
        agent.close()
