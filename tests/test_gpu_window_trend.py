"""The window-trend kernels (csrc/window_trend.hip) against the exact oracle of tests/_exact.py,
slot by slot: the one-shot op over a wrapped ring, DeviceWindowSet.export_trend after every
refresh of its incremental paths, LongWindowSet.export_trend over a filling and a wrapped
device ring, the argument checks, and GpuAgent end to end.

Per (series, slot): count, min and max are EQUAL bit for bit (-0.0 and +0.0 told apart), the
mean is within ``_exact.mean_bound(ex, s, sum_group=1)`` - fp64 adds only, one rounding to
fp32 - and an empty slot is count 0 with three NaNs. Every buffer is filled with -1 before
the call that writes it, so a slot the kernel left out shows."""

import numpy as np
import pytest

import _exact
from _window_exports import _assert_trend, _bits

pytestmark = pytest.mark.gpu

PCT = (50.0, 90.0, 99.0)  # exact_stats wants percentiles; the trend has none


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


# series taken per ring stride: 16 = the first families (zeroes, ties, ramps, sparse, inf), 11 =
# the last (all NaN, constant, denormal, the +-inf ends), 5 = wide .. ties, 1 = the +-inf ends
_SLICES = {1: slice(22, 23), 5: slice(2, 7), 11: slice(12, 23), 16: slice(0, 16), 23: slice(0, 23)}
SHAPES = [(1, 64, 8), (63, 64, 64), (64, 64, 64), (65, 128, 8), (4096, 4096, 64), (4096, 4096, 1024)]


@pytest.mark.parametrize("stride", [1, 5, 11, 16, 23])
@pytest.mark.parametrize("head_kind", ["n", "n+1", "wrapped"])
@pytest.mark.parametrize("n,window,P", SHAPES)
def test_window_trend_one_shot(native, cuda, n, window, P, head_kind, stride):
    """The smallest shapes that reach c = 1, a partial first and last slot, the ring wrap, a
    row stride that is no multiple of 4, more slots than rows, and both kernels (a wave or a
    workgroup per slot)."""
    import torch

    from rocmdash.ops.window_trend import window_trend

    head = {"n": n, "n+1": n + 1, "wrapped": 3 * window - 1}[head_kind]
    x = np.array(_one_shot_rows(n)[_SLICES[stride]])  # a writable copy of the shared rows
    assert x.shape == (stride, n)
    got = window_trend(torch.from_numpy(x).to(cuda), P, head=head, window=window)
    torch.cuda.synchronize()
    full = _assert_trend(got.cpu().numpy(), x.T, head, window, P)
    assert full == len({r // (window // P) for r in range(head - n, head)})


def test_window_trend_one_workgroup_streams_many_rows(native, cuda):
    """window 2^17, P = 8: 16384 rows x 3 series per workgroup, far more rows than threads."""
    import torch

    from rocmdash.ops.window_trend import window_trend

    W, P = 1 << 17, 8
    rng = np.random.default_rng(17)
    x = np.stack([_exact.family(f, rng, 0, W, W) for f in ("normal_nan", "wide", "zeroes")])
    head = W + 12345
    got = window_trend(torch.from_numpy(x).to(cuda), P, head=head, window=W)
    torch.cuda.synchronize()
    assert _assert_trend(got.cpu().numpy(), x.T, head, W, P) == P + 1


def test_window_trend_is_deterministic(native, cuda):
    import torch

    from rocmdash.ops.window_trend import window_trend

    x = torch.from_numpy(np.array(_one_shot_rows(4096)[:16])).to(cuda)
    a = window_trend(x, 8, head=5000, window=4096)
    b = window_trend(x, 8, head=5000, window=4096)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


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


def _assert_all_empty(t):
    assert (t[:, :, 3] == 0).all() and np.isnan(t[:, :, :3]).all()


@pytest.mark.parametrize("P", [8, 64])
@pytest.mark.parametrize("W", [64, 4096])
def test_export_trend_after_every_refresh(native, cuda, W, P):
    """Two rings (11 + 5 series) in one DeviceWindowSet, pull mode: the trend is exact after
    EVERY refresh - a full sort, then one row, none, a few, 255 / 256 / 257 - each ring's series
    at its offset; its counts, minima and maxima add up to the statistics of the same refresh;
    a full column keeps its bits while the window slides; no state, no slots."""
    import torch

    from rocmdash.ops.window_trend import trend_geometry

    nat = native
    nat.set_pinned_host_rings(True)
    nat.set_pull_mode(True)
    rs = _Rings(nat, W, (11, 5))
    S, c = rs.S, W // P
    out = torch.empty((S, 8), device=cuda)
    dst = torch.empty((S, P + 1, 4), device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    steps = [W + 3, 1, 1, 0, 2, 17, 255, 256, 257, 1]

    dst.fill_(-1.0)
    rs.dws.export_trend(P, dst.data_ptr(), stream)  # no refresh yet
    torch.cuda.synchronize()
    _assert_all_empty(dst.cpu().numpy())

    prev, stable = None, 0
    for i, add in enumerate(steps):
        rs.push(add)
        rs.dws.refresh(out.data_ptr(), stream, *PCT)
        dst.fill_(-1.0)
        rs.dws.export_trend(P, dst.data_ptr(), stream)
        torch.cuda.synchronize()
        got, st = dst.cpu().numpy(), out.cpu().numpy()
        win = rs.window()
        _assert_trend(got, win, rs.t, W, P, what=f"after +{add} rows")
        # against the statistics of the same refresh
        np.testing.assert_array_equal(got[:, :, 3].sum(axis=1), st[:, _exact.COUNT])
        with np.errstate(invalid="ignore"):
            np.testing.assert_array_equal(np.fmin.reduce(got[:, :, 0], axis=1), st[:, _exact.MIN])
            np.testing.assert_array_equal(np.fmax.reduce(got[:, :, 1], axis=1), st[:, _exact.MAX])
        # a column that is full in both refreshes keeps its bits
        _, ranges = trend_geometry(rs.t, len(win), W, P)
        last = (rs.t - 1) // c
        if prev is not None and add < c:
            plast, pranges, pgot = prev
            for j, (b, e) in enumerate(ranges):
                jp = j + (last - plast)
                if e - b == c and 0 <= jp <= P and pranges[jp, 1] - pranges[jp, 0] == c:
                    assert (pranges[jp] == (b, e)).all()
                    np.testing.assert_array_equal(_bits(got[:, j]), _bits(pgot[:, jp]), err_msg=f"column [{b}, {e})")
                    stable += 1
        prev = (last, ranges, got)
    assert stable >= P  # columns were compared

    rs.dws.invalidate()
    dst.fill_(-1.0)
    rs.dws.export_trend(P, dst.data_ptr(), stream)
    torch.cuda.synchronize()
    _assert_all_empty(dst.cpu().numpy())


@pytest.mark.parametrize("P", [8, 256])
@pytest.mark.parametrize("W", [1024, 65536])
def test_long_window_export_trend(native, cuda, W, P):
    """One ring of 12 series in a LongWindowSet: before any refresh, after the first fill
    (a window that is not full yet, then full), after +100 rows, and after enough rows to wrap
    the device ring - exact against a host mirror, the counts adding up to the refresh's."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    cap = 2 * W
    ring = nat.SeriesRing(12, cap)
    lw = nat.LongWindowSet(W, 0)
    lw.add_ring(ring)
    out = torch.empty((12, 8), device=cuda)
    dst = torch.empty((12, P + 1, 4), device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    dst.fill_(-1.0)
    lw.export_trend(P, dst.data_ptr(), stream)
    torch.cuda.synchronize()
    _assert_all_empty(dst.cpu().numpy())

    rng = np.random.default_rng(W + P)
    rows = np.zeros((0, 12), np.float32)
    t = 0
    for add in (W // 2 + 5, W // 2 + 32, 100, W + W // 4 + 7):
        x = _exact.family_rows(rng, t, add, W, width=12, first=1, blips=(t + 9,))
        ring.push_many(x, np.arange(t + 1, t + 1 + add, dtype=np.uint64))
        rows = np.concatenate([rows, x])[-W:]
        t += add
        lw.refresh(out.data_ptr(), stream, *PCT)
        dst.fill_(-1.0)
        lw.export_trend(P, dst.data_ptr(), stream)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        _assert_trend(got, rows, t, W, P, what=f"after +{add} rows (t = {t})")
        np.testing.assert_array_equal(got[:, :, 3].sum(axis=1), out.cpu().numpy()[:, _exact.COUNT])
    assert lw.stats()["rows_lost"] == 0


def test_trend_entries_reject_before_launching(native, cuda):
    """A bad column count, more columns than rows, more than 65536 rows per column, a
    rows_per_col that does not divide the depth, n past the depth and a null dst raise with
    nothing launched: the -1-filled buffer is untouched."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    dst = torch.full((4, 2049, 4), -1.0, device=cuda)
    W = 64
    ring_mem = torch.zeros((2 * W, 4), device=cuda)

    def one_shot(P=8, c=None, depth=2 * W, n=W, head=W, d=None, base=None, stride=4, cols=4):
        nat.trend_ring(ring_mem.data_ptr() if base is None else base, stride, cols, depth, head, n, P,
                       W // P if c is None and P else (c or 0), dst.data_ptr() if d is None else d, stream)

    bad = [dict(P=0), dict(P=6), dict(P=2048), dict(P=128),  # 128 > W: no row per column
           dict(P=8, c=1 << 17, depth=1 << 20),  # W / P > 65536
           dict(c=3), dict(n=2 * W + 1, head=4 * W), dict(n=W, head=W - 1), dict(c=4, n=W), dict(d=0), dict(base=0),
           dict(stride=0), dict(stride=65, cols=65), dict(cols=5), dict(cols=0), dict(depth=96)]
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
                ws.export_trend(P, dst.data_ptr(), stream)
        with pytest.raises(RuntimeError):
            ws.export_trend(8, 0, stream)
    with pytest.raises(RuntimeError):
        big.export_trend(128, dst.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool((dst == -1).all())  # nothing ran
    one_shot(n=0, head=0)  # a valid call: every slot empty
    torch.cuda.synchronize()
    _assert_all_empty(dst.cpu().numpy().reshape(-1)[:4 * 9 * 4].reshape(4, 9, 4))


@pytest.mark.parametrize("long", [False, True])
def test_agent_window_trend_end_to_end(native, cuda, long):
    """GpuAgent on the GPU, short and long window sets: window_trend() in stream order after
    refresh() equals the reference over each ring's host window and adds up to its counts."""
    import torch

    from rocmdash.config import SamplerConfig
    from rocmdash.ops.window_trend import window_trend_reference
    from rocmdash.runtime.agent import GpuAgent

    W = 1 << 16 if long else 256
    cfg = SamplerConfig(window=W, ring_capacity=W if long else 1024)
    agent = GpuAgent(0, source="synthetic", counters="synthetic", cfg=cfg)
    try:
        assert type(agent.dws).__name__ == ("LongWindowSet" if long else "DeviceWindowSet")
        agent.prefill(W + 44 if long else 300)
        for more in (0, 1, 7):
            for _ in range(more):
                agent.sample()
            st = agent.refresh()
            tr = agent.window_trend(8)
            torch.cuda.synchronize()
            got = tr.cpu().numpy()
            assert got.shape == (len(agent.series), 9, 4)
            s = 0
            for i, r in enumerate(agent.rings):
                rows, _ = agent.window_host(i)
                _assert_trend(got[s:s + r.width], rows, r.head, W, 8, what=f"ring {i}")
                want = window_trend_reference(rows, r.head, W, 8)
                np.testing.assert_array_equal(_bits(got[s:s + r.width, :, [0, 1, 3]]), _bits(want[:, :, [0, 1, 3]]))
                s += r.width
            np.testing.assert_array_equal(got[:, :, 3].sum(axis=1), st.cpu().numpy()[:, 7])
            assert got[:, :, 3].sum(axis=1).max() == W
        assert agent.window_trend(8) is tr  # the buffer is reused
        with pytest.raises(ValueError):
            agent.window_trend(6)
    finally:
        agent.close()
