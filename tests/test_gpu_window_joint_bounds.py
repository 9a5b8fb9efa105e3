"""The window joint-histogram kernel (csrc/window_joint.hip) on bounds that are NOT evenly
spaced, where its guess of a sample's bin is far off and the walk over the lane's LDS column of
the bounds is what makes the counts right - the joint kernel's own copy of the rule that
test_gpu_long_window_bucket_bounds.py drives in csrc/long_window_buckets.hip, with the same
bounds and samples (tests/_bucket_bounds.py) and NaN among them. Here the walk is divergent
per lane while the two shuffles after it must be reached by every lane; a lane whose sample is
NaN keeps a stale bin and must still hand out "no bin"; and the two series of a pair have
bounds of different families, so one lane walks 30 bins while its partner walks none.

Every comparison is exact integer equality with ``window_joint_reference`` and
``bucket_ring_reference``; every destination is filled with -1 before the call that writes it
and has one spare pair that must stay -1. Each test prints how many counts it compared and
asserts the number its shapes give."""

import numpy as np
import pytest

import _bucket_bounds as bb
from _bucket_bounds import _launch_inputs, _shifts, _walkers, _windows
from _window_exports import _assert_joint

pytestmark = pytest.mark.gpu

PCT = (50.0, 90.0, 99.0)


def _report(request, compared):
    print(f"[joint] {request.node.name}: {compared} count comparisons")


def _pairs(cols, K):
    """K = 1: the first column with the last. K = 8: a pair and its transpose and one series in
    several pairs; with 2 columns the two possible pairs named four times each; with 5 and 7
    columns eight distinct pairs - at stride 5 and 7 more than the lanes of a row, the second
    owner pass."""
    if K == 1:
        return [(0, cols - 1)]
    if cols == 2:
        return [(0, 1), (1, 0)] * 4
    if cols < 8:
        out = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1), (0, cols - 1), (cols - 1, 1)]
    else:
        out = [(1, 3), (3, 1), (1, 7), (7, 3), (14, 4), (4, 6), (cols - 1, 0), (0, cols - 1)]
    assert len(set(out)) == 8
    return out


@pytest.mark.parametrize("B", bb.JOINT_B)
@pytest.mark.parametrize("depth,stride,cols", bb.JOINT_RINGS)
def test_joint_ring_on_uneven_bounds(native, cuda, request, depth, stride, cols, B):
    """One pair per two lanes (2 x 2), the counter ring's stride (5), eight distinct pairs for
    seven lanes of a row (7 x 7: the second owner pass), columns nobody reads (12 x 7), idle tail
    lanes (23), 64 workgroups adding onto the same cells and a wrapped window as two blocks
    (4096 x 64). The inputs, launches and windows are the heatmap's: neighbouring lanes - and so
    the two series of every pair - hold the bounds of different families, every bounds family
    meets every sample family, every second launch has NaN in 5 % of the samples; K rotates over
    1 and 8. Where B >= 16, the windows of more than one row need the walk. ``bucket_ring`` on
    the same ring, window and bounds holds the first copy of the rule to this one: without NaN
    a pair's row sums are the de-cumulated counts of ``a``, its column sums those of ``b``."""
    import torch

    from rocmdash.ops.window_buckets import bucket_ring_reference

    stream = torch.cuda.current_stream().cuda_stream
    B1 = B + 1
    dst = torch.empty((9, B1, B1), dtype=torch.int32, device=cuda)
    counts = torch.empty((cols + 1, B1), dtype=torch.float64, device=cuda)
    shifts, windows = _shifts(cols), _windows(depth)
    compared, expected, walked, with_nan, nan_pairs, marginals, seen_k = 0, 0, set(), 0, 0, 0, set()
    for i, (o, s) in enumerate(shifts):
        clean, rows, bounds, names = _launch_inputs(depth, stride, cols, B, i, o, s)
        assert names[0][0] != names[1][0]
        with_nan += int(np.isnan(rows[:, :cols]).sum() > np.isnan(clean[:, :cols]).sum())
        ring = torch.from_numpy(rows).to(cuda)
        bd = torch.from_numpy(bounds).to(cuda)
        for w, (kind, head, n) in enumerate(windows):
            K = (1, 8)[(i + w) % 2]
            pairs = _pairs(cols, K)
            seen_k.add((K, i % 2))
            for a, b in pairs:  # bounds go by column: a pair never has one family twice
                assert names[a][0] != names[b][0], (a, b, names[a], names[b])
            if B >= 16 and n > 1:
                walked |= _walkers(clean, bounds, names, head, n)  # NaN only removes samples
            dst.fill_(-1)
            counts.fill_(-1.0)
            native.joint_ring(ring.data_ptr(), stride, cols, depth, head, n, pairs, bd.data_ptr(), B, dst.data_ptr(), stream)
            native.bucket_ring(ring.data_ptr(), stride, cols, depth, head, n, bd.data_ptr(), B, counts.data_ptr(), stream)
            torch.cuda.synchronize()
            got, le = dst.cpu().numpy(), counts.cpu().numpy()
            slots = np.arange(head - n, head, dtype=np.int64) & (depth - 1)
            win = rows[slots, :cols]
            where = f"{kind}, K {K}, offset {o}, shift {s}: {[(names[a], names[b]) for a, b in pairs]}"
            want = _assert_joint(got[:K], win, pairs, bounds, what=where)  # and: a pair's cells sum to the rows valid in both
            assert (got[K:] == -1).all(), f"{where}: wrote past the last pair"
            np.testing.assert_array_equal(le[:cols], bucket_ring_reference(rows, head, n, bounds).astype(np.float64), err_msg=where)
            bins = np.diff(le[:cols], axis=1, prepend=0.0)  # [cols, B + 1]: the le counts de-cumulated
            has_nan = np.isnan(win).any(axis=0)
            for k, (a, b) in enumerate(pairs):
                if (b, a) in pairs:
                    np.testing.assert_array_equal(got[k], got[pairs.index((b, a))].T, err_msg=f"{where}: pair {k} / its transpose")
                nan_pairs += int(has_nan[a] and has_nan[b] and got[k].sum() > 0)
                if not (has_nan[a] or has_nan[b]):
                    np.testing.assert_array_equal(got[k].sum(axis=1), bins[a], err_msg=f"{where}: pair {k}, rows / bucket_ring")
                    np.testing.assert_array_equal(got[k].sum(axis=0), bins[b], err_msg=f"{where}: pair {k}, columns / bucket_ring")
                    marginals += 1
            compared += want.size
            expected += K * B1 * B1
    if B >= 16:
        assert walked == set(bb.WALKS), walked
    assert 0 < with_nan <= len(shifts) // 2
    assert seen_k == {(1, 0), (1, 1), (8, 0), (8, 1)}  # both K with and without NaN
    assert nan_pairs > 0 and marginals > 0  # NaN columns paired with each other; pairs held to bucket_ring
    assert compared == expected == sum((1, 8)[(i + w) % 2] for i in range(len(shifts)) for w in range(4)) * B1 * B1
    _report(request, compared)


@pytest.mark.parametrize("B", [16, 31])
@pytest.mark.parametrize("long", [True, False])
def test_export_joint_on_uneven_bounds(native, cuda, request, long, B):
    """``LongWindowSet.export_joint`` at W = 1024 and ``DeviceWindowSet.export_joint`` at W = 512
    over two rings of 8 and 13 series fed the ``_exact`` families, one pair inside each ring and
    its transpose: after every refresh - a part-filled window, a full one, +1 row, none, +100,
    +257 and enough to wrap the device ring - with bounds on the samples of that very window, one
    ulp beside them, geometric, and of a span that overflows, series by series; the four series
    of the pairs have one kind each."""
    import torch

    W = 1024 if long else 512
    rings = bb.ExportRings(native, W, long, seed=B)
    S = rings.S
    # narrow_nan x ties in the first ring, sparse3 x narrow_negative in the second (series 8 ..)
    pairs = [(1, 6), (6, 1), (12, 19), (19, 12)]
    assert {bb.EXPORT_KINDS[s % 4] for s in (1, 6, 12, 19)} == set(bb.EXPORT_KINDS)
    K, B1 = len(pairs), B + 1
    out = torch.empty((S, 8), device=cuda)
    dst = torch.empty((K + 1, B1, B1), dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    steps = bb.export_steps(W)
    compared = 0
    for add in steps:
        rings.push(add)
        rings.ws.refresh(out.data_ptr(), stream, *PCT)
        win = rings.window()
        b = rings.bounds(B)
        bd = torch.from_numpy(b).to(cuda)
        dst.fill_(-1)
        rings.ws.export_joint(pairs, bd.data_ptr(), B, dst.data_ptr(), stream)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        want = _assert_joint(got[:K], win, pairs, b, what=f"after +{add} rows (t = {rings.t})")
        assert (got[K] == -1).all()
        np.testing.assert_array_equal(got[0], got[1].T)
        np.testing.assert_array_equal(got[2], got[3].T)
        assert want[0].sum() > 0 and want[2].sum() > 0
        compared += want.size
    assert rings.t > 2 * W  # the device ring (W rows of the long set, 2 W of the other) wrapped
    assert compared == len(steps) * K * B1 * B1
    _report(request, compared)
