"""The window-heatmap kernels (csrc/window_heatmap.hip) on bounds that are NOT evenly spaced,
where their guess of a sample's bin is far off and the walk over the lane's LDS column of the
bounds is what makes the counts right - the heatmap's own copy of the rule that
test_gpu_long_window_bucket_bounds.py drives in csrc/long_window_buckets.hip, with the same
bounds and samples (tests/_bucket_bounds.py) and, here, NaN among them. Around the walk the
heatmap flushes a run length (a plain add in the one-wave kernel, an LDS atomic in the
eight-wave one), flushes a slot's last run after the loop, and cuts slots at absolute row
numbers, so a long run of one bin crosses slots.

Every comparison is exact integer equality with ``window_heatmap_reference`` and
``bucket_ring_reference``; every destination is filled with -1 before the call that writes it
and has one spare series that must stay -1. Each test prints how many counts it compared and
asserts the number its shapes give."""

import numpy as np
import pytest

import _bucket_bounds as bb
from _bucket_bounds import _launch_inputs, _shifts, _walkers, _windows
from _window_exports import _assert_heatmap

pytestmark = pytest.mark.gpu

PCT = (50.0, 90.0, 99.0)


def _report(request, compared):
    print(f"[heatmap] {request.node.name}: {compared} count comparisons")


@pytest.mark.parametrize("B", bb.HEATMAP_B)
@pytest.mark.parametrize("depth,stride,cols,P,c", bb.HEATMAP_RINGS)
def test_heatmap_ring_on_uneven_bounds(native, cuda, request, depth, stride, cols, P, c, B):
    """A wave per slot (a single series, pieces of 63 floats, columns nobody reads, slots of 16
    rows in which a run ends almost every time) and eight waves per slot (idle tail lanes at
    stride 23, a lane per series at 64). Neighbouring lanes hold the bounds of different
    families in one launch, launch after launch every bounds family meets every sample family,
    and every second launch has NaN in 5 % of the samples. Windows: one row; part-filled;
    full at a head inside a column, so all P + 1 slots are used and the oldest and the newest
    are partial; wrapped and part-filled at a head past 2^32. Where B >= 16, the windows of
    more than one row need the walk. ``bucket_ring`` on the same ring, window and bounds holds
    the first copy of the rule to this one: the heatmap summed over slots and cumulated over
    bins is its counts."""
    import torch

    from rocmdash.ops.window_buckets import bucket_ring_reference
    from rocmdash.ops.window_heatmap import window_heatmap_reference
    from rocmdash.ops.window_trend import trend_geometry

    stream = torch.cuda.current_stream().cuda_stream
    dst = torch.empty((cols + 1, P + 1, B + 1), dtype=torch.int32, device=cuda)
    counts = torch.empty((cols + 1, B + 1), dtype=torch.float64, device=cuda)
    shifts, windows = _shifts(cols), _windows(depth)
    assert windows[2][2] == depth and windows[2][1] % c != 0  # the full window: P + 1 slots, two of them partial
    compared, walked, with_nan = 0, set(), 0
    for i, (o, s) in enumerate(shifts):
        clean, rows, bounds, names = _launch_inputs(depth, stride, cols, B, i, o, s)
        if cols > 1:
            assert names[0][0] != names[1][0]
        with_nan += int(np.isnan(rows[:, :cols]).sum() > np.isnan(clean[:, :cols]).sum())
        ring = torch.from_numpy(rows).to(cuda)
        bd = torch.from_numpy(bounds).to(cuda)
        for kind, head, n in windows:
            if B >= 16 and n > 1:
                walked |= _walkers(clean, bounds, names, head, n)  # NaN only removes samples
            dst.fill_(-1)
            counts.fill_(-1.0)
            native.heatmap_ring(ring.data_ptr(), stride, cols, depth, head, n, P, c, bd.data_ptr(), B, dst.data_ptr(), stream)
            native.bucket_ring(ring.data_ptr(), stride, cols, depth, head, n, bd.data_ptr(), B, counts.data_ptr(), stream)
            torch.cuda.synchronize()
            got, le = dst.cpu().numpy(), counts.cpu().numpy()
            slots = np.arange(head - n, head, dtype=np.int64) & (depth - 1)
            want = window_heatmap_reference(rows[slots, :cols], head, depth, P, bounds)
            want_le = bucket_ring_reference(rows, head, n, bounds)
            assert want.shape == (cols, P + 1, B + 1) and want_le.shape == (cols, B + 1)
            if n == depth:  # every slot is used, the oldest and the newest in part
                rows_of = np.diff(trend_geometry(head, n, depth, P)[1], axis=1)[:, 0]
                assert (rows_of > 0).all() and rows_of[0] < c and rows_of[-1] < c and rows_of.sum() == n
            for col in range(cols):  # by column: the message names the families
                where = f"{kind}, column {col}: {names[col]}, offset {o}, shift {s}"
                np.testing.assert_array_equal(got[col], want[col], err_msg=where)
                np.testing.assert_array_equal(le[col], want_le[col].astype(np.float64), err_msg=f"{where}: bucket_ring")
            np.testing.assert_array_equal(np.cumsum(got[:cols].sum(axis=1), axis=1).astype(np.float64), le[:cols],
                                          err_msg=f"{kind}: the heatmap's slots summed and cumulated / bucket_ring")
            assert (got[cols] == -1).all() and (le[cols] == -1).all(), f"{kind}: wrote past the last series"
            compared += want.size + want_le.size
    if B >= 16:
        assert walked == set(bb.WALKS), walked
    assert 0 < with_nan <= len(shifts) // 2
    assert compared == len(shifts) * len(windows) * cols * (P + 2) * (B + 1)
    _report(request, compared)


@pytest.mark.parametrize("B", [16, 63])
@pytest.mark.parametrize("long", [True, False])
def test_export_heatmap_on_uneven_bounds(native, cuda, request, long, B):
    """``LongWindowSet.export_heatmap`` at W = 1024 and ``DeviceWindowSet.export_heatmap`` at
    W = 512 over two rings of 8 and 13 series fed the ``_exact`` families, P = 8: after every
    refresh - a part-filled window, a full one, +1 row, none, +100, +257 and enough to wrap the
    device ring - with bounds on the samples of that very window, one ulp beside them, geometric,
    and of a span that overflows, series by series. The counts are the reference's, the bins of a
    slot sum to ``export_trend``'s count, and a second export of the same window into another
    buffer agrees bit for bit."""
    import torch

    W, P = 1024 if long else 512, 8
    rings = bb.ExportRings(native, W, long, seed=B)
    S = rings.S
    out = torch.empty((S, 8), device=cuda)
    dsts = [torch.empty((S + 1, P + 1, B + 1), dtype=torch.int32, device=cuda) for _ in range(2)]
    trend = torch.empty((S, P + 1, 4), device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    steps = bb.export_steps(W)
    compared = 0
    for add in steps:
        rings.push(add)
        rings.ws.refresh(out.data_ptr(), stream, *PCT)
        win = rings.window()
        b = rings.bounds(B)
        bd = torch.from_numpy(b).to(cuda)
        trend.fill_(-1.0)
        for d in dsts:
            d.fill_(-1)
            rings.ws.export_heatmap(P, bd.data_ptr(), B, d.data_ptr(), stream)
        rings.ws.export_trend(P, trend.data_ptr(), stream)
        torch.cuda.synchronize()
        got = dsts[0].cpu().numpy()
        want = _assert_heatmap(got[:S], win, rings.t, W, P, b, what=f"after +{add} rows (t = {rings.t})")
        np.testing.assert_array_equal(got[:S].sum(axis=2), trend.cpu().numpy()[:, :, 3])
        assert (got[S] == -1).all()
        assert torch.equal(dsts[0], dsts[1])
        compared += want.size
    assert rings.t > 2 * W  # the device ring (W rows of the long set, 2 W of the other) wrapped
    assert want.sum(axis=(1, 2)).max() == W
    assert compared == len(steps) * S * (P + 1) * (B + 1)
    _report(request, compared)
