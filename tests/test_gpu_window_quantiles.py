"""The window-quantile kernels (csrc/window_quantiles.hip) against the exact oracle of
tests/_exact.py, slot by slot: the one-shot op over a wrapped ring on both paths (the LDS sort
and the radix select) and at their boundary, DeviceWindowSet.export_quantiles after every
refresh, LongWindowSet.export_quantiles over a filling and a wrapped device ring, the argument
checks, and GpuAgent end to end.

Per (series, slot, percentile): the count is EQUAL; with no valid sample the values are NaN;
where ``frac == 0`` or ``x0 == x1`` the output IS the order statistic; otherwise it is within
one fp32 ulp of the oracle and inside ``[x0, x1]``. The one comparison left out: an
interpolation between order statistics of which one is infinite, and only in the series that
hold infinities by construction. Every buffer is filled with -1 before the call that writes it."""

import numpy as np
import pytest

import _exact
from _window_exports import _assert_quantiles
from test_gpu_window_trend import SHAPES, _Rings, _SLICES, _assert_all_empty, _bits, _one_shot_rows

pytestmark = pytest.mark.gpu

PCT = (50.0, 90.0, 99.0)
ENDS_PCT = (0.0, 37.5, 100.0)  # the ends are selections
# the series of _one_shot_rows that hold infinities: the inf family and the +-inf ends
_NONFINITE = (_exact.INF_SERIES, len(_exact.FAMILIES) + 1)


def _nonfinite_in(sl):
    """Local indices, within the slice ``sl`` of _one_shot_rows, of the series with infinities."""
    idx = list(range(*sl.indices(len(_exact.FAMILIES) + 2)))
    return tuple(idx.index(g) for g in _NONFINITE if g in idx)


def _slots(head, n, c):
    """Non-empty slots of the window [head - n, head) with c rows per column."""
    return (head - 1) // c - (head - n) // c + 1 if n else 0


def _run_one_shot(cuda, x, P, pct, head, window, nonfinite_ok):
    import torch

    from rocmdash.ops.window_quantiles import window_quantiles

    got = window_quantiles(torch.from_numpy(x).to(cuda), P, pct=pct, head=head, window=window)
    torch.cuda.synchronize()
    S, n = x.shape
    made = _assert_quantiles(got.cpu().numpy(), x.T, head, window, P, pct, nonfinite_ok)
    assert made >= _slots(head, n, window // P) * 3 * (S - len(nonfinite_ok))
    return got


@pytest.mark.parametrize("pct", [PCT, ENDS_PCT])
@pytest.mark.parametrize("stride", [1, 5, 11, 16, 23])
@pytest.mark.parametrize("head_kind", ["n", "n+1", "wrapped"])
@pytest.mark.parametrize("n,window,P", SHAPES)
def test_window_quantiles_one_shot(native, cuda, n, window, P, head_kind, stride, pct):
    """The trend test's shapes: c = 1, a partial first and last slot, the ring wrap, a row
    stride that is no multiple of 4, more slots than rows; the default percentiles and a set
    whose ends are selections."""
    head = {"n": n, "n+1": n + 1, "wrapped": 3 * window - 1}[head_kind]
    x = np.array(_one_shot_rows(n)[_SLICES[stride]])
    assert x.shape == (stride, n)
    _run_one_shot(cuda, x, P, pct, head, window, _nonfinite_in(_SLICES[stride]))


@pytest.mark.parametrize("stride", [5, 23])
def test_window_quantiles_sort_in_a_workgroup(native, cuda, stride):
    """512 rows per column: 5 series are sorted by 4 waves, 23 by 16."""
    x = np.array(_one_shot_rows(4096)[_SLICES[stride]])
    _run_one_shot(cuda, x, 8, PCT, 3 * 4096 - 1, 4096, _nonfinite_in(_SLICES[stride]))


def test_window_quantiles_path_boundary(native, cuda):
    """The largest column the LDS sort takes and the smallest the radix select takes, on the
    same rows: 17 series, so the sort cuts the ring into groups and the select into two."""
    T = native.QUANTILE_SORT_MAX_ROWS
    P = 8
    x = np.array(_one_shot_rows(2 * T * P)[:17])
    nonfinite = _nonfinite_in(slice(0, 17))
    for c in (T, 2 * T):
        W = c * P
        _run_one_shot(cuda, np.ascontiguousarray(x[:, -W:]), P, PCT, W + c // 2 + 3, W, nonfinite)


def test_window_quantiles_one_workgroup_streams_many_rows(native, cuda):
    """window 2^17, P = 8: 16384 rows x 3 series per workgroup, far more rows than threads."""
    W, P = 1 << 17, 8
    rng = np.random.default_rng(17)
    x = np.stack([_exact.family(f, rng, 0, W, W) for f in ("normal_nan", "wide", "zeroes")])
    head = W + 12345
    _run_one_shot(cuda, x, P, PCT, head, W, ())
    assert _slots(head, W, W // P) == P + 1


def test_window_quantiles_full_columns_of_65536_rows(native, cuda):
    """window 2^19, P = 8, head a multiple of c: full slots of 65536 rows. A constant series
    puts every sample in one bin of every digit (a bin has to count to 65536), a ramp spreads."""
    W, P = 1 << 19, 8
    rng = np.random.default_rng(19)
    x = np.stack([_exact.family(f, rng, 0, W, W) for f in ("constant", "ramp_up")])
    got = _run_one_shot(cuda, x, P, PCT, 3 * W, W, ())
    g = got.cpu().numpy()
    assert (g[:, 1:, 3] == 65536).all() and (g[:, 0, 3] == 0).all()


def test_window_quantiles_is_deterministic(native, cuda):
    import torch

    from rocmdash.ops.window_quantiles import window_quantiles

    x = torch.from_numpy(np.array(_one_shot_rows(4096)[:16])).to(cuda)
    a = window_quantiles(x, 8, head=5000, window=4096)
    b = window_quantiles(x, 8, head=5000, window=4096)
    T = native.QUANTILE_SORT_MAX_ROWS
    y = torch.from_numpy(np.array(_one_shot_rows(16 * T)[:16])).to(cuda)
    c = window_quantiles(y, 8, head=16 * T + 77, window=16 * T)
    d = window_quantiles(y, 8, head=16 * T + 77, window=16 * T)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    np.testing.assert_array_equal(_bits(c.cpu().numpy()), _bits(d.cpu().numpy()))


def _assert_within_trend(q, t, what="", nonfinite_ok=()):
    """count bit-equal to the trend's; every percentile inside the slot's trend [min, max] - but
    for a series in ``nonfinite_ok``, whose interpolation against an infinite order statistic
    is NaN by the arithmetic (inf - inf)."""
    np.testing.assert_array_equal(_bits(q[:, :, 3]), _bits(t[:, :, 3]), err_msg=f"{what}: count")
    has = t[:, :, 3] > 0
    for k in range(3):
        v = q[:, :, k]
        assert np.isnan(v[~has]).all(), what
        inside = (v >= t[:, :, 0]) & (v <= t[:, :, 1])
        for s in nonfinite_ok:
            inside[s] |= np.isnan(v[s]) & ~(np.isfinite(t[s, :, 0]) & np.isfinite(t[s, :, 1]))
        assert inside[has].all(), f"{what}: p{k} outside the trend's band: series / slot {np.argwhere(has & ~inside)}"


@pytest.mark.parametrize("P", [8, 64])
@pytest.mark.parametrize("W", [64, 4096])
def test_export_quantiles_after_every_refresh(native, cuda, W, P):
    """Two rings (11 + 5 series) in one DeviceWindowSet, pull mode: exact after EVERY refresh,
    each ring's series at its offset; the count is the trend's of the same refresh and every
    percentile lies in its band; a full column keeps its bits while the window slides; no
    state, no slots."""
    import torch

    from rocmdash.ops.window_trend import trend_geometry

    nat = native
    nat.set_pinned_host_rings(True)
    nat.set_pull_mode(True)
    rs = _Rings(nat, W, (11, 5))
    S, c = rs.S, W // P
    out = torch.empty((S, 8), device=cuda)
    dst = torch.empty((S, P + 1, 4), device=cuda)
    trend = torch.empty((S, P + 1, 4), device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    steps = [W + 3, 1, 1, 0, 2, 17, 255, 256, 257, 1]
    nonfinite = (_exact.INF_SERIES,)  # _Rings feeds series s family s

    dst.fill_(-1.0)
    rs.dws.export_quantiles(P, dst.data_ptr(), stream, *PCT)  # no refresh yet
    torch.cuda.synchronize()
    _assert_all_empty(dst.cpu().numpy())

    prev, stable = None, 0
    for i, add in enumerate(steps):
        rs.push(add)
        rs.dws.refresh(out.data_ptr(), stream, *PCT)
        dst.fill_(-1.0)
        trend.fill_(-1.0)
        rs.dws.export_quantiles(P, dst.data_ptr(), stream, *PCT)
        rs.dws.export_trend(P, trend.data_ptr(), stream)
        torch.cuda.synchronize()
        got, tr = dst.cpu().numpy(), trend.cpu().numpy()
        win = rs.window()
        what = f"after +{add} rows"
        made = _assert_quantiles(got, win, rs.t, W, P, PCT, nonfinite, what=what)
        assert made >= _slots(rs.t, len(win), c) * 3 * (S - 1)
        _assert_within_trend(got, tr, what, nonfinite)
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
    rs.dws.export_quantiles(P, dst.data_ptr(), stream, *PCT)
    torch.cuda.synchronize()
    _assert_all_empty(dst.cpu().numpy())


@pytest.mark.parametrize("P", [8, 256])
@pytest.mark.parametrize("W", [1024, 65536])
def test_long_window_export_quantiles(native, cuda, W, P):
    """One ring of 12 series in a LongWindowSet: before any refresh, after the first fill (a
    window that is not full yet, then full), after +100 rows, and after enough rows to wrap the
    device ring - exact against a host mirror, the count the trend's, full columns stable."""
    import torch

    from rocmdash.ops.window_trend import trend_geometry

    nat = native
    nat.set_pinned_host_rings(True)
    ring = nat.SeriesRing(12, 2 * W)
    lw = nat.LongWindowSet(W, 0)
    lw.add_ring(ring)
    c = W // P
    out = torch.empty((12, 8), device=cuda)
    dst = torch.empty((12, P + 1, 4), device=cuda)
    trend = torch.empty((12, P + 1, 4), device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    dst.fill_(-1.0)
    lw.export_quantiles(P, dst.data_ptr(), stream, *PCT)
    torch.cuda.synchronize()
    _assert_all_empty(dst.cpu().numpy())

    rng = np.random.default_rng(W + P)
    rows = np.zeros((0, 12), np.float32)
    t, prev, stable = 0, None, 0
    for add in (W // 2 + 5, W // 2 + 32, 100, W + W // 4 + 7):
        x = _exact.family_rows(rng, t, add, W, width=12, first=1, blips=(t + 9,))  # no series with infinities
        ring.push_many(x, np.arange(t + 1, t + 1 + add, dtype=np.uint64))
        rows = np.concatenate([rows, x])[-W:]
        t += add
        lw.refresh(out.data_ptr(), stream, *PCT)
        dst.fill_(-1.0)
        trend.fill_(-1.0)
        lw.export_quantiles(P, dst.data_ptr(), stream, *PCT)
        lw.export_trend(P, trend.data_ptr(), stream)
        torch.cuda.synchronize()
        got, tr = dst.cpu().numpy(), trend.cpu().numpy()
        what = f"after +{add} rows (t = {t})"
        made = _assert_quantiles(got, rows, t, W, P, PCT, (), what=what)
        assert made == _slots(t, len(rows), c) * 3 * 12
        _assert_within_trend(got, tr, what)
        np.testing.assert_array_equal(got[:, :, 3].sum(axis=1), out.cpu().numpy()[:, _exact.COUNT])
        _, ranges = trend_geometry(t, len(rows), W, P)
        last = (t - 1) // c
        if prev is not None:
            plast, pranges, pgot = prev
            for j, (b, e) in enumerate(ranges):
                jp = j + (last - plast)
                if e - b == c and 0 <= jp <= P and pranges[jp, 1] - pranges[jp, 0] == c:
                    assert (pranges[jp] == (b, e)).all()
                    np.testing.assert_array_equal(_bits(got[:, j]), _bits(pgot[:, jp]), err_msg=f"column [{b}, {e})")
                    stable += 1
        prev = (last, ranges, got)
    assert stable >= P  # columns were compared
    assert lw.stats()["rows_lost"] == 0


def test_quantile_entries_reject_before_launching(native, cuda):
    """The trend entries' bad arguments, a NaN percentile and one above 100 raise with nothing
    launched: the -1-filled buffer is untouched."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    dst = torch.full((4, 2049, 4), -1.0, device=cuda)
    W = 64
    ring_mem = torch.zeros((2 * W, 4), device=cuda)

    def one_shot(P=8, c=None, depth=2 * W, n=W, head=W, d=None, base=None, stride=4, cols=4, pct=PCT):
        nat.quantile_ring(ring_mem.data_ptr() if base is None else base, stride, cols, depth, head, n, P,
                          W // P if c is None and P else (c or 0), dst.data_ptr() if d is None else d, stream, *pct)

    bad = [dict(P=0), dict(P=6), dict(P=2048), dict(P=128),  # 128 > W: no row per column
           dict(P=8, c=1 << 17, depth=1 << 20),  # W / P > 65536
           dict(c=3), dict(n=2 * W + 1, head=4 * W), dict(n=W, head=W - 1), dict(c=4, n=W), dict(d=0), dict(base=0),
           dict(stride=0), dict(stride=65, cols=65), dict(cols=5), dict(cols=0), dict(depth=96),
           dict(pct=(50.0, float("nan"), 99.0)), dict(pct=(50.0, 90.0, 100.5)), dict(pct=(-1.0, 90.0, 99.0)),
           dict(pct=(float("inf"), 90.0, 99.0))]
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
                ws.export_quantiles(P, dst.data_ptr(), stream, *PCT)
        with pytest.raises(RuntimeError):
            ws.export_quantiles(8, 0, stream, *PCT)
        with pytest.raises(RuntimeError):
            ws.export_quantiles(8, dst.data_ptr(), stream, 50.0, float("nan"), 99.0)
        with pytest.raises(RuntimeError):
            ws.export_quantiles(8, dst.data_ptr(), stream, 50.0, 90.0, 101.0)
    with pytest.raises(RuntimeError):
        big.export_quantiles(128, dst.data_ptr(), stream, *PCT)
    torch.cuda.synchronize()
    assert bool((dst == -1).all())  # nothing ran
    one_shot(n=0, head=0)  # a valid call: every slot empty
    torch.cuda.synchronize()
    _assert_all_empty(dst.cpu().numpy().reshape(-1)[:4 * 9 * 4].reshape(4, 9, 4))


@pytest.mark.parametrize("long", [False, True])
def test_agent_window_quantiles_end_to_end(native, cuda, long):
    """GpuAgent on the GPU, short and long window sets: window_quantiles() in stream order
    after refresh() is exact over each ring's host window, equals the reference and carries
    the trend's counts."""
    import torch

    from rocmdash.config import SamplerConfig
    from rocmdash.ops.window_quantiles import window_quantiles_reference
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
            qt = agent.window_quantiles(8)
            tr = agent.window_trend(8)
            torch.cuda.synchronize()
            got = qt.cpu().numpy()
            assert got.shape == (len(agent.series), 9, 4)
            s = 0
            for i, r in enumerate(agent.rings):
                rows, _ = agent.window_host(i)
                made = _assert_quantiles(got[s:s + r.width], rows, r.head, W, 8, agent.pct, (), what=f"ring {i}")
                assert made == _slots(r.head, len(rows), W // 8) * 3 * r.width
                want = window_quantiles_reference(rows, r.head, W, 8, agent.pct)
                np.testing.assert_array_equal(_bits(got[s:s + r.width, :, 3]), _bits(want[:, :, 3]))
                s += r.width
            _assert_within_trend(got, tr.cpu().numpy(), "agent")
            np.testing.assert_array_equal(got[:, :, 3].sum(axis=1), st.cpu().numpy()[:, 7])
        assert agent.window_quantiles(8) is qt  # the buffer is reused
        with pytest.raises(ValueError):
            agent.window_quantiles(6)
    finally:
        agent.close()
