"""The streaming le-bucket kernel (csrc/long_window_buckets.hip) on bounds that are NOT evenly
spaced, where its guess of a sample's bin is far off and the walk over the lane's LDS column
of the bounds is what makes the counts right: geometric bounds and their mirror image, a span
that overflows, denormal bounds, runs of consecutive floats, two far outliers round such a
run, and bounds on the samples and one ulp beside them (tests/_bucket_bounds.py). The samples
visit every bin, sit on the bounds and one ulp beside them, stay in one bin for long runs, and
are the ``_exact`` families every other kernel is held to.

Every comparison is exact integer equality with ``bucket_ring_reference`` /
``window_buckets_reference``; every destination is filled with -1 before the call that writes
it and has one spare row that must stay -1. Each test prints how many counts it compared and
asserts the number its shapes give."""

import numpy as np
import pytest

import _bucket_bounds as bb
import _exact
from _bucket_bounds import _ring_inputs, _shifts, _walkers, _windows

pytestmark = pytest.mark.gpu

COUNT = 7  # the window statistics' count column
F = len(bb.BOUNDS)


def _report(request, compared):
    print(f"[buckets] {request.node.name}: {compared} count comparisons")


RINGS = [(1024, 1, 1), (1024, 3, 3), (1024, 12, 7), (1024, 13, 13), (4096, 64, 64)]


@pytest.mark.parametrize("B", [1, 2, 3, 16, 63])
@pytest.mark.parametrize("depth,stride,cols", RINGS)
def test_bucket_ring_on_uneven_bounds(native, cuda, request, depth, stride, cols, B):
    """One workgroup (1024 x 1), pieces of 63, 60 and 52 floats with a short last one, columns
    nobody reads (12 x 7), 64 workgroups adding onto the same bins (4096 x 64). Neighbouring
    lanes hold the bounds of different families in one launch - the [k][lane] layout of the
    bounds in LDS - and launch after launch every bounds family meets every sample family.
    Where B >= 16, the windows of more than one row need the walk: every walking family shows
    its precondition on the samples of the window itself."""
    import torch

    from rocmdash.ops.window_buckets import bucket_ring_reference

    stream = torch.cuda.current_stream().cuda_stream
    dst = torch.empty((cols + 1, B + 1), dtype=torch.float64, device=cuda)
    shifts, windows = _shifts(cols), _windows(depth)
    compared, walked = 0, set()
    for o, s in shifts:
        rows, bounds, names = _ring_inputs(depth, stride, cols, B, o, s)
        if cols > 1:
            assert names[0][0] != names[1][0]
        ring = torch.from_numpy(rows).to(cuda)
        bd = torch.from_numpy(bounds).to(cuda)
        for kind, head, n in windows:
            if B >= 16 and n > 1:
                walked |= _walkers(rows, bounds, names, head, n)
            dst.fill_(-1.0)
            native.bucket_ring(ring.data_ptr(), stride, cols, depth, head, n, bd.data_ptr(), B, dst.data_ptr(), stream)
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            want = bucket_ring_reference(rows, head, n, bounds)
            assert want.shape == (cols, B + 1) and want[:, -1].max() <= n
            for c in range(cols):  # by column: the message names the families
                np.testing.assert_array_equal(got[c], want[c].astype(np.float64),
                                              err_msg=f"{kind}, column {c}: {names[c]}, offset {o}, shift {s}")
            assert (got[cols] == -1).all(), f"{kind}: wrote past the last series"
            compared += want.size
    if B >= 16:
        assert walked == set(bb.WALKS), walked
    assert compared == len(shifts) * len(windows) * cols * (B + 1)
    _report(request, compared)


def _series_bounds(x, name, B):
    """[S, B]: the family's bounds for every series (from its own samples where it has such)."""
    if name in bb.STATIC:
        return np.ascontiguousarray(np.tile(bb.STATIC[name](B), (len(x), 1)))
    return np.stack([bb.bounds_for(name, B, x[s]) for s in range(len(x))])


@pytest.mark.parametrize("B", [16, 63])
@pytest.mark.parametrize("n", [4097, 32768])
def test_both_kernels_agree_on_uneven_bounds(native, cuda, request, n, B):
    """The streamed counts (float64) and the sorted window's (float32) of the same samples and
    bounds, each equal to the reference and so to each other: the 21 ``_exact`` families, a
    constant row and a row with -inf and +inf at its ends, under every bounds family."""
    import torch

    from rocmdash.ops.window_buckets import long_window_buckets, window_buckets, window_buckets_reference

    x = bb.one_shot_rows(n)
    S = len(x)
    assert S == len(_exact.FAMILIES) + 2
    xd = torch.from_numpy(np.array(x)).to(cuda)
    compared = 0
    for name in bb.BOUNDS:
        b = _series_bounds(x, name, B)
        streamed, short = long_window_buckets(xd, b), window_buckets(xd, b)
        torch.cuda.synchronize()
        assert streamed.dtype == torch.float64 and short.dtype == torch.float32
        streamed, short = streamed.cpu().numpy(), short.cpu().numpy()
        want = window_buckets_reference(x, b)
        assert want[:, -1].max() == n
        np.testing.assert_array_equal(streamed, want.astype(np.float64), err_msg=f"{name}: streamed")
        np.testing.assert_array_equal(short.astype(np.float64), want.astype(np.float64), err_msg=f"{name}: sorted")
        np.testing.assert_array_equal(streamed, short.astype(np.float64), err_msg=name)
        compared += 2 * want.size
    assert compared == 2 * F * S * (B + 1)
    _report(request, compared)


class _Mirror:
    """Everything pushed, oldest first."""

    def __init__(self, width):
        self.rows = np.zeros((0, width), np.float32)

    def push(self, x):
        self.rows = np.concatenate([self.rows, x])

    def window(self, W):
        return self.rows[-W:]


class _LwRings:
    """Two rings of 8 and 13 series (two segments, unaligned rows) fed the 21 families."""

    def __init__(self, nat, W, cap, seed):
        self.W = W
        self.ra, self.rb = nat.SeriesRing(8, cap), nat.SeriesRing(13, cap)
        self.m = _Mirror(21)
        self.rng = np.random.default_rng(seed)
        self.t = 0

    def add_to(self, s):
        s.add_ring(self.ra)
        s.add_ring(self.rb)

    def push(self, k):
        if not k:
            return
        x = _exact.family_rows(self.rng, self.t, k, self.W, width=21, blips=(5, self.W + 8))
        ts = np.arange(self.t, self.t + k, dtype=np.uint64)
        self.ra.push_many(np.ascontiguousarray(x[:, :8]), ts)
        self.rb.push_many(np.ascontiguousarray(x[:, 8:]), ts)
        self.m.push(x)
        self.t += k


EXPORT_KINDS = ("on_samples", "between", "geometric", "huge_span")


@pytest.mark.parametrize("B", [16, 63])
def test_long_window_export_buckets_on_uneven_bounds(native, cuda, request, B):
    """``LongWindowSet.export_buckets`` at W = 1024 over two rings of 8 and 13 series fed the
    ``_exact`` families: after every refresh - a part-filled window, a full one, +1 row, none,
    +100, +257 and enough to wrap the device ring - with bounds on the samples of that very
    window, one ulp beside them, geometric, and of a span that overflows, series by series.
    The counts are the reference's, the last column is the refresh's count, and a second
    export of the same window into another buffer agrees bit for bit."""
    import torch

    from rocmdash.ops.window_buckets import window_buckets_reference

    nat = native
    nat.set_pinned_host_rings(True)
    W, S = 1024, 21
    rings = _LwRings(nat, W, 2 * W, seed=B)
    lw = nat.LongWindowSet(W, 0)
    rings.add_to(lw)
    out = torch.empty((S, 8), device=cuda)
    dsts = [torch.empty((S + 1, B + 1), dtype=torch.float64, device=cuda) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    steps = [W // 2 + 5, W // 2 + 32, 1, 0, 100, 257, W + W // 4 + 7]
    compared = 0
    for add in steps:
        rings.push(add)
        lw.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
        x = np.ascontiguousarray(rings.m.window(W).T)
        b = np.stack([bb.bounds_for(EXPORT_KINDS[s % 4], B, x[s]) for s in range(S)])
        bd = torch.from_numpy(b).to(cuda)
        for d in dsts:
            d.fill_(-1.0)
            lw.export_buckets(bd.data_ptr(), B, d.data_ptr(), stream)
        torch.cuda.synchronize()
        got = dsts[0].cpu().numpy()
        want = window_buckets_reference(x, b)
        np.testing.assert_array_equal(got[:S], want.astype(np.float64), err_msg=f"after +{add} rows (t = {rings.t})")
        np.testing.assert_array_equal(got[:S, B], out.cpu().numpy()[:, COUNT].astype(np.float64))
        assert (got[S] == -1).all()
        assert torch.equal(dsts[0].view(torch.int64), dsts[1].view(torch.int64))
        compared += want.size
    assert rings.t > 2 * W and lw.stats()["rows_lost"] == 0  # the device ring of W rows wrapped
    assert want[:, B].max() == W
    assert compared == len(steps) * S * (B + 1)
    _report(request, compared)
