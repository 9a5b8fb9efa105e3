"""The window joint-histogram kernel (csrc/window_joint.hip) against the numpy reference of
rocmdash.ops.window_joint (itself checked against a per-row loop in test_window_joint.py): the
one-shot op over a wrapped ring, a window that many workgroups share, DeviceWindowSet.export_joint
after every refresh, LongWindowSet.export_joint over a filling, a full and a wrapped device
ring, the argument checks, and GpuAgent end to end.

Counts are integers: every comparison is exact equality. Every buffer is filled with -1 before
the call that writes it, so a cell the kernel left out shows."""

import os

import numpy as np
import pytest

import _exact
from _window_exports import _assert_joint

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURE = os.path.join(ROOT, "tests", "fixtures", "mi355x_capture.npz")
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


F = {name: i for i, name in enumerate(_exact.FAMILIES)}
# series taken per ring stride. 2: two NaN families (pairwise validity); 5: NaNs, +-inf, a
# constant; 7: those and ties; 16 / 23: the first families in order (23: + constant, + ends)
_TAKE = {2: [F["narrow_nan"], F["wide_nan"]],
         5: [F["wide_nan"], F["ties_nan"], F["inf"], 21, 22],
         7: [F["narrow_nan"], F["wide_nan"], F["ties_nan"], F["normal_nan"], F["inf"], 21, F["ties"]],
         16: list(range(16)), 23: list(range(23))}


def _pairs(stride, K):
    """K = 1: one pair. K = 8: a pair and its transpose, one series in several pairs, NaN families
    with NaN families; at stride 2 the two possible pairs named four times each; at stride 7
    eight distinct pairs for seven lanes of a row - the second owner pass."""
    if K == 1:
        return [(0, stride - 1)]
    if stride == 2:
        return [(0, 1), (1, 0)] * 4
    if stride < 8:
        out = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1), (0, stride - 1), (stride - 1, 1)]
    else:  # 1 narrow_nan, 3 wide_nan, 7 ties_nan, 14 inf, 4 zeroes, 6 ties, the last: all_nan / the +-inf ends
        out = [(1, 3), (3, 1), (1, 7), (7, 3), (14, 4), (4, 6), (stride - 1, 0), (0, stride - 1)]
    assert len(set(out)) == 8
    return out


SIZES = [(1, 8), (63, 64), (64, 64), (65, 128), (4096, 4096)]
HEADS = ["n", "n+1", "wrapped"]
STRIDES = [2, 5, 7, 16, 23]
BUCKETS = [1, 16, 31]
# The cross product thinned: every (size, head kind, stride) runs once, with B, the kind of
# bounds and K rotating - over the file each stride meets each B, both kinds of bounds and both K.
ONE_SHOT = [(n, W, HEADS[h], STRIDES[s], BUCKETS[(i + h + s) % 3], "even" if (i + h) // 3 % 2 == 0 else "quantile",
             (1, 8)[(i + s) % 2])
            for i, (n, W) in enumerate(SIZES) for h in range(3) for s in range(5)]


def test_one_shot_cases_cover_the_cross():
    for stride in STRIDES:
        for B in BUCKETS:
            assert {c[5] for c in ONE_SHOT if c[3] == stride and c[4] == B} == {"even", "quantile"}, (stride, B)
            assert {c[6] for c in ONE_SHOT if c[3] == stride and c[4] == B} == {1, 8}, (stride, B)
        for n, _ in SIZES:
            assert {c[2] for c in ONE_SHOT if c[3] == stride and c[0] == n} == set(HEADS)


@pytest.mark.parametrize("n,window,head_kind,stride,B,kind,K", ONE_SHOT)
def test_window_joint_one_shot(native, cuda, n, window, head_kind, stride, B, kind, K):
    """The smallest shapes that reach one row, a last piece that is not full, the ring wrap, one
    pair per two lanes (stride 2), the counter ring's stride 5, more pairs than lanes of a row
    (stride 7, K = 8: the second owner pass), and idle tail lanes (stride 23)."""
    import torch

    from rocmdash.ops.window_joint import check_joint_bounds, window_joint

    head = {"n": n, "n+1": n + 1, "wrapped": 3 * window - 1}[head_kind]
    x = np.array(_one_shot_rows(n)[_TAKE[stride]])  # a writable copy of the shared rows
    assert x.shape == (stride, n)
    bounds = check_joint_bounds((_even_bounds if kind == "even" else _quantile_bounds)(x, B), stride)
    pairs = _pairs(stride, K)
    out = torch.full((len(pairs), B + 1, B + 1), -1, dtype=torch.int32, device=cuda)
    got = window_joint(torch.from_numpy(x).to(cuda), pairs, bounds, head=head, window=window, out=out)
    assert got is out
    torch.cuda.synchronize()
    want = _assert_joint(got.cpu().numpy(), x.T, pairs, bounds, what=f"stride {stride} head {head}")
    for k, (a, b) in enumerate(pairs):  # a pair and its transpose in one call
        if (b, a) in pairs:
            np.testing.assert_array_equal(want[k], want[pairs.index((b, a))].T)


def test_window_joint_many_workgroups(native, cuda):
    """window 2^17 x 4 series, wrapped: 128 workgroups over two blocks add onto the same cells;
    the same bits on a second run, and each pair's total is the rows valid in both series."""
    import torch

    from rocmdash.ops.window_joint import window_joint

    W, B = 1 << 17, 16
    rng = np.random.default_rng(17)
    x = np.stack([_exact.family(f, rng, 0, W, W) for f in ("normal_nan", "wide_nan", "zeroes", "narrow")])
    bounds = _quantile_bounds(x, B)
    pairs = [(0, 1), (1, 0), (0, 3), (2, 3), (3, 1)]
    head = 3 * W - 1000
    xd = torch.from_numpy(x).to(cuda)
    fill = lambda: torch.full((len(pairs), B + 1, B + 1), -1, dtype=torch.int32, device=cuda)  # noqa: E731
    got = window_joint(xd, pairs, bounds, head=head, window=W, out=fill())
    again = window_joint(xd, pairs, bounds, head=head, window=W, out=fill())
    torch.cuda.synchronize()
    want = _assert_joint(got.cpu().numpy(), x.T, pairs, bounds)
    np.testing.assert_array_equal(again.cpu().numpy(), want)
    both = np.count_nonzero(~np.isnan(x[0]) & ~np.isnan(x[1]))
    assert 0 < both < W and want[0].sum() == both and want[3].sum() == W


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


@pytest.mark.parametrize("W", [64, 4096])
def test_export_joint_after_every_refresh(native, cuda, W):
    """Three rings (11 + 5 + 3 series) in one DeviceWindowSet, pairs in the first two and none in
    the third: the joint histograms equal the reference after EVERY refresh while the window
    fills, is full and wraps the device ring; all zeroes without state."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    nat.set_pull_mode(True)
    rs = _Rings(nat, W, (11, 5, 3))
    S, B = rs.S, 16
    # ring 0: narrow_nan x wide_nan, its transpose, ties_nan x zeroes; ring 1 (series 11 ..): sparse2 x sparse3,
    # blip x inf, inf x all_nan (never both valid), sparse3 x sparse2
    pairs = [(1, 3), (3, 1), (7, 4), (11, 12), (13, 14), (14, 15), (12, 11)]
    bounds = _mixed_bounds(np.random.default_rng(W), S, B)
    bd = torch.from_numpy(bounds).to(cuda)
    out = torch.empty((S, 8), device=cuda)
    dst = torch.empty((len(pairs), B + 1, B + 1), dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    dst.fill_(-1)
    rs.dws.export_joint(pairs, bd.data_ptr(), B, dst.data_ptr(), stream)  # no refresh yet
    torch.cuda.synchronize()
    assert bool((dst == 0).all())

    for add in [W // 2, W // 2 + 3, 1, 0, 2, 17, W - 20, 255, 1]:
        rs.push(add)
        rs.dws.refresh(out.data_ptr(), stream, *PCT)
        dst.fill_(-1)
        rs.dws.export_joint(pairs, bd.data_ptr(), B, dst.data_ptr(), stream)
        torch.cuda.synchronize()
        want = _assert_joint(dst.cpu().numpy(), rs.window(), pairs, bounds, what=f"after +{add} rows (t = {rs.t})")
        assert (want[5] == 0).all() and want[0].sum() > 0
    assert rs.t > 2 * W  # the device ring of 2 W rows wrapped

    only = [(12, 15)]  # one ring with a pair, two without
    one = torch.full((1, B + 1, B + 1), -1, dtype=torch.int32, device=cuda)
    rs.dws.export_joint(only, bd.data_ptr(), B, one.data_ptr(), stream)
    torch.cuda.synchronize()
    _assert_joint(one.cpu().numpy(), rs.window(), only, bounds)

    rs.dws.invalidate()
    dst.fill_(-1)
    rs.dws.export_joint(pairs, bd.data_ptr(), B, dst.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool((dst == 0).all())


def test_long_window_export_joint(native, cuda):
    """One ring of 12 series in a LongWindowSet at its smallest window (2^10): all zeroes before
    any refresh; after the first fill (a window that is not full yet, then full), after +100 rows,
    and after enough rows to wrap the device ring the joint histograms equal the reference over a
    host mirror."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    W, B = 1 << 10, 31
    ring = nat.SeriesRing(12, 2 * W)
    lw = nat.LongWindowSet(W, 0)
    lw.add_ring(ring)
    rng = np.random.default_rng(W)
    bounds = _mixed_bounds(rng, 12, B)
    bd = torch.from_numpy(bounds).to(cuda)
    pairs = [(0, 2), (2, 0), (0, 6), (3, 6), (1, 11), (5, 4), (10, 9), (8, 7)]  # families 1 .. 12
    out = torch.empty((12, 8), device=cuda)
    dst = torch.empty((len(pairs), B + 1, B + 1), dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    dst.fill_(-1)
    lw.export_joint(pairs, bd.data_ptr(), B, dst.data_ptr(), stream)
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
        lw.export_joint(pairs, bd.data_ptr(), B, dst.data_ptr(), stream)
        torch.cuda.synchronize()
        _assert_joint(dst.cpu().numpy(), rows, pairs, bounds, what=f"after +{add} rows (t = {t})")
    assert lw.stats()["rows_lost"] == 0


def test_joint_entries_reject_before_launching(native, cuda):
    """K = 0 and 9, B = 0 and 32, a == b, an index at cols, a pair across rings, the ring
    conditions of bucket_ring and a null or misaligned pointer raise with nothing launched or
    written: the -1-filled buffer is untouched."""
    import torch

    nat = native
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    dst = torch.full((8 * 32 * 32 + 64,), -1, dtype=torch.int32, device=cuda)
    W = 64
    ring_mem = torch.zeros((2 * W, 4), device=cuda)
    bd = torch.arange(16 * 32, dtype=torch.float32, device=cuda)  # ascending for any B

    def one_shot(pairs=((0, 1),), depth=2 * W, n=W, head=W, d=None, base=None, stride=4, cols=4, B=16, b=None):
        nat.joint_ring(ring_mem.data_ptr() if base is None else base, stride, cols, depth, head, n, list(pairs),
                       bd.data_ptr() if b is None else b, B, dst.data_ptr() if d is None else d, stream)

    bad = [dict(pairs=()), dict(pairs=[(0, 1)] * 9), dict(pairs=[(2, 2)]), dict(pairs=[(0, 4)]), dict(pairs=[(4, 0)]),
           dict(pairs=[(0, 3)], cols=3), dict(B=0), dict(B=32), dict(b=0), dict(d=0), dict(base=0),
           dict(d=dst.data_ptr() + 2), dict(d=dst.data_ptr() + 1), dict(n=2 * W + 1, head=4 * W), dict(n=W, head=W - 1),
           dict(stride=0), dict(stride=65, cols=65), dict(cols=5), dict(cols=0), dict(depth=96)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            one_shot(**kw)

    dws = nat.DeviceWindowSet(W, 0)
    lw = nat.LongWindowSet(1 << 10, 0)
    keep = []
    for ws, cap in ((dws, 8 * W), (lw, 1 << 11)):
        for w in (11, 5):
            keep.append(nat.SeriesRing(w, cap))
            ws.add_ring(keep[-1])
    for ws in (dws, lw):
        for pairs in ([], [(0, 1)] * 9, [(3, 3)], [(0, 16)], [(16, 0)], [(10, 11)], [(12, 2)], [(0, 1), (1, 11)]):
            with pytest.raises(RuntimeError):
                ws.export_joint(pairs, bd.data_ptr(), 16, dst.data_ptr(), stream)
        for b, B, d in ((bd.data_ptr(), 0, dst.data_ptr()), (bd.data_ptr(), 32, dst.data_ptr()), (0, 16, dst.data_ptr()),
                        (bd.data_ptr(), 16, 0), (bd.data_ptr(), 16, dst.data_ptr() + 2)):
            with pytest.raises(RuntimeError):
                ws.export_joint([(0, 1)], b, B, d, stream)
    torch.cuda.synchronize()
    assert bool((dst == -1).all())  # nothing ran
    one_shot(pairs=[(0, 1), (1, 0)], n=0, head=0)  # a valid call: every cell zero
    dws.export_joint([(11, 12)], bd.data_ptr(), 31, dst.data_ptr() + 4 * 2 * 17 * 17, stream)  # no refresh yet: zeroes
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    used = 2 * 17 * 17 + 32 * 32
    assert (got[:used] == 0).all() and (got[used:] == -1).all()


@pytest.mark.parametrize("long", [False, True])
def test_agent_window_joint_on_a_recording(native, cuda, long):
    """GpuAgent replaying the MI355X capture, short and long window sets: window_joint() in
    stream order after refresh() equals the reference over window_host() of the pair's ring, with
    the default pairs and bounds and with given ones; the buffer is reused for the same pairs."""
    import torch

    from rocmdash.config import SamplerConfig
    from rocmdash.runtime.agent import GpuAgent

    W = 1 << 16 if long else 256
    agent = GpuAgent(0, source="replay", replay=CAPTURE, cfg=SamplerConfig(window=W, ring_capacity=W if long else 1024))
    try:
        assert type(agent.dws).__name__ == ("LongWindowSet" if long else "DeviceWindowSet")
        agent.prefill(W + 44 if long else 300)
        defaults = agent.default_joint_pairs()
        assert 1 <= len(defaults) <= 4
        bounds = agent.default_bucket_bounds(16)
        starts = np.cumsum([0] + [r.width for r in agent.rings])

        def check(got, pairs, b):
            for k, (a, c) in enumerate(pairs):
                i = int(np.searchsorted(starts, a, side="right")) - 1
                rows, _ = agent.window_host(i)
                rows = np.asarray(rows, np.float32).reshape(-1, agent.rings[i].width)
                s = int(starts[i])
                _assert_joint(got[k:k + 1], rows, [(a - s, c - s)], b[s:s + agent.rings[i].width], what=f"pair {k}")

        first = None
        for more in (0, 1, 7):
            for _ in range(more):
                agent.sample()
            agent.refresh()
            j = agent.window_joint()
            torch.cuda.synchronize()
            got = j.cpu().numpy()
            assert got.shape == (len(defaults), 17, 17) and got.dtype == np.int32
            check(got, defaults, bounds)
            assert got.sum(axis=(1, 2)).max() > 0
            first = j if first is None else first
            assert j is first  # the buffer is reused
        given = [(2, 1), (1, 2), (0, 5)]  # power x activity and its transpose, edge x junction temperature
        custom = np.ascontiguousarray(bounds[:, ::2])
        other = agent.window_joint(given, custom)
        torch.cuda.synchronize()
        assert other is not first and tuple(other.shape) == (3, custom.shape[1] + 1, custom.shape[1] + 1)
        check(other.cpu().numpy(), given, custom)
        assert agent.window_joint(list(given), custom) is other
        with pytest.raises(ValueError):
            agent.window_joint([(0, len(agent.series) - 1)] if len(agent.rings) > 1 else [(0, 0)])
    finally:
        agent.close()
