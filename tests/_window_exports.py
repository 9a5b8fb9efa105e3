"""What the window-export tests share: the "hold ``got`` to the reference" helpers of the feature
tests (test_gpu_window_trend.py and its siblings import them back from here), a host mirror of
one ring, ``check_all_exports`` - every export of a window set against the CPU references of
``rocmdash.ops`` over the mirrors' windows - and the ring-state scenarios of
test_window_exports_scenarios.py (CPU: which states a schedule reaches) and
test_gpu_window_exports.py (GPU: the exports in those states).

The comparison rules are the feature tests' own: counts and integer sums EQUAL, min and max equal
bit for bit, the mean within ``_exact.mean_bound(..., sum_group=1)``, a percentile the order
statistic itself or within one fp32 ulp of the oracle and inside ``[x0, x1]``. No tolerance is
introduced here.

Plain numpy at import time (torch and the native module only inside the GPU helpers); imported
like ``_exact`` and ``_bucket_bounds``.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import _bucket_bounds
import _exact
import _window_xcorr

PCT = (50.0, 90.0, 99.0)


# ---- the feature tests' asserts, bodies as they were in those files -------------------------
def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _assert_trend(got, rows, head, W, P, what=""):
    """``got`` [S, P + 1, 4] against the oracle over ``rows`` [n, S] = rows head - n .. head - 1.
    Returns the number of non-empty slots."""
    from rocmdash.ops.window_trend import trend_geometry

    got = np.asarray(got)
    n, S = rows.shape
    assert got.dtype == np.float32 and got.shape == (S, P + 1, 4), (got.shape, got.dtype)
    _, ranges = trend_geometry(head, n, W, P)
    first, full = head - n, 0
    for j, (b, e) in enumerate(ranges):
        g = got[:, j]
        where = f"{what} slot {j} rows [{b}, {e}) head {head} n {n} W {W} P {P}"
        if e <= b:
            assert (g[:, 3] == 0).all() and np.isnan(g[:, :3]).all(), f"{where}: not empty: {g}"
            continue
        full += 1
        ex = _exact.exact_stats(np.ascontiguousarray(rows[b - first:e - first]), PCT)
        np.testing.assert_array_equal(g[:, 3], ex.count.astype(np.float32), err_msg=f"{where}: count")
        for s in range(S):
            if not ex.nv[s]:
                assert np.isnan(g[s, :3]).all(), f"{where} series {s}: {g[s]} with no valid sample"
                continue
            assert _bits(g[s, 0]) == _bits(ex.min[s]), f"{where} series {s}: min {g[s, 0]!r} != {ex.min[s]!r}"
            assert _bits(g[s, 1]) == _bits(ex.max[s]), f"{where} series {s}: max {g[s, 1]!r} != {ex.max[s]!r}"
            if not (np.isfinite(ex.mean[s]) and np.isfinite(ex.mean_abs[s])):
                continue
            err, bound = abs(float(g[s, 2]) - float(ex.mean[s])), _exact.mean_bound(ex, s, sum_group=1)
            assert err <= bound, f"{where} series {s}: mean {g[s, 2]!r} vs {ex.mean[s]!r}: |diff| {err:.3e} > {bound:.3e}"
    return full


def _assert_quantiles(got, rows, head, W, P, pct, nonfinite_ok=(), what=""):
    """``got`` [S, P + 1, 4] against the oracle over ``rows`` [n, S] = rows head - n .. head - 1.
    Returns the number of (series, slot, percentile) comparisons made; a comparison is left
    out only for a series in ``nonfinite_ok`` interpolating against an infinite order statistic."""
    from rocmdash.ops.window_trend import trend_geometry

    got = np.asarray(got)
    n, S = rows.shape
    assert got.dtype == np.float32 and got.shape == (S, P + 1, 4), (got.shape, got.dtype)
    _, ranges = trend_geometry(head, n, W, P)
    first, made = head - n, 0
    for j, (b, e) in enumerate(ranges):
        g = got[:, j]
        where = f"{what} slot {j} rows [{b}, {e}) head {head} n {n} W {W} P {P}"
        if e <= b:
            assert (g[:, 3] == 0).all() and np.isnan(g[:, :3]).all(), f"{where}: not empty: {g}"
            continue
        ex = _exact.exact_stats(np.ascontiguousarray(rows[b - first:e - first]), pct)
        np.testing.assert_array_equal(g[:, 3], ex.count.astype(np.float32), err_msg=f"{where}: count")
        for s in range(S):
            for q in range(3):
                have = g[s, q]
                if not ex.nv[s]:
                    assert np.isnan(have), f"{where} series {s}: {g[s]} with no valid sample"
                    made += 1
                    continue
                x0, x1, f, want = ex.x0[s, q], ex.x1[s, q], ex.frac[s, q], ex.percentile[s, q]
                msg = (f"{where} series {s}: p{ex.pct[q]:g} = {have!r}, oracle {want!r} (x0 {x0!r} at "
                       f"{ex.pos[s, 2 * q]}, x1 {x1!r} at {ex.pos[s, 2 * q + 1]}, frac {f!r}, nv {ex.nv[s]})")
                if f == 0 or x0 == x1:
                    assert _exact._same(have, x0), msg
                elif not (np.isfinite(x0) and np.isfinite(x1)):
                    assert s in nonfinite_ok, msg + ": an infinite order statistic in a finite series"
                    continue
                else:
                    assert _exact._within_one_ulp(have, want), msg
                    assert x0 <= have <= x1, msg + ": outside [x0, x1]"
                made += 1
    return made


def _assert_heatmap(got, rows, head, W, P, bounds, what=""):
    """``got`` [S, P + 1, B + 1] against the reference over ``rows`` [n, S] = rows head - n .. head - 1."""
    from rocmdash.ops.window_heatmap import window_heatmap_reference

    got = np.asarray(got)
    want = window_heatmap_reference(rows, head, W, P, bounds)
    assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, got.dtype, want.shape)
    if not np.array_equal(got, want):
        s, j, k = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError(f"{what} head {head} n {len(rows)} W {W} P {P} B {bounds.shape[1]}: "
                             f"{np.count_nonzero(got != want)} counts differ, first series {s} slot {j} bin {k}: "
                             f"{got[s, j, k]} != {want[s, j, k]}; slot: {got[s, j]} != {want[s, j]}")
    return want


def _assert_joint(got, rows, pairs, bounds, what=""):
    """``got`` [K, B + 1, B + 1] against the reference over ``rows`` [n, S]; the cells of a pair
    sum to the rows valid in both series."""
    from rocmdash.ops.window_joint import window_joint_reference

    got = np.asarray(got)
    want = window_joint_reference(rows, pairs, bounds)
    assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, got.dtype, want.shape)
    if not np.array_equal(got, want):
        k, i, j = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError(f"{what} n {len(rows)} B {bounds.shape[1]} pairs {pairs}: "
                             f"{np.count_nonzero(got != want)} cells differ, first pair {k} = {pairs[k]} cell ({i}, {j}): "
                             f"{got[k, i, j]} != {want[k, i, j]}; sums {got[k].sum()} != {want[k].sum()}")
    rows = np.asarray(rows)
    for k, (a, b) in enumerate(pairs):
        assert want[k].sum() == np.count_nonzero(~np.isnan(rows[:, a]) & ~np.isnan(rows[:, b]))
    return want


def _assert_autocorr(got, x, scale, L, span=None, what=""):
    """``got`` [S, L + 1, 4] against the reference over ``x`` [S, n]."""
    from rocmdash.ops.window_autocorr import window_autocorr_reference

    got = np.asarray(got)
    want = window_autocorr_reference(x.T, scale, L, span)
    assert got.dtype == np.int64 and got.shape == want.shape, (got.shape, got.dtype, want.shape)
    if not np.array_equal(got, want):
        s, k, j = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError(f"{what} n {x.shape[1]} L {L}: {np.count_nonzero(got != want)} words differ, first series {s} "
                             f"lag {k} word {j}: {got[s, k, j]} != {want[s, k, j]}")
    assert (want[:, 0, 1] == want[:, 0, 2]).all()
    return want


def _assert_periods(got, rows, scale, head, W, P, L, span, what=""):
    """``got`` [S, P + 1, L + 1, 4] against the reference over ``rows`` [n, S] = rows head - n .. head - 1."""
    from rocmdash.ops.window_periods import window_periods_reference

    got = np.asarray(got)
    want = window_periods_reference(rows, scale, head, W, P, L, span)
    assert got.dtype == np.int64 and got.shape == want.shape, (got.shape, got.dtype, want.shape)
    if not np.array_equal(got, want):
        s, j, k, i = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError(f"{what} head {head} n {len(rows)} W {W} P {P} L {L} span {span}: "
                             f"{np.count_nonzero(got != want)} words differ, first series {s} slot {j} lag {k} word {i}: "
                             f"{got[s, j, k, i]} != {want[s, j, k, i]}")
    return want


def _assert_counts(got, x, bounds, what=""):
    from rocmdash.ops.window_buckets import window_buckets_reference

    got = np.asarray(got)
    assert got.dtype == np.float32
    want = window_buckets_reference(x, bounds)
    np.testing.assert_array_equal(got.astype(np.int64), want, err_msg=what)
    np.testing.assert_array_equal(got, want.astype(np.float32), err_msg=what)  # whole numbers, nothing else
    return want


# The long buckets' and the excursions' tests compare in line (no helper to lift): the same
# equalities, named.
def _assert_long_counts(got, x, bounds, what=""):
    """LongWindowSet.export_buckets: float64 [S, B + 1] EQUAL to the reference over ``x`` [S, n]."""
    from rocmdash.ops.window_buckets import window_buckets_reference

    got = np.asarray(got)
    assert got.dtype == np.float64
    want = window_buckets_reference(x, bounds)
    np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=what)
    return want


def _assert_excursions(got, rows, thresholds, what=""):
    """int32 [S, K, 8] EQUAL to the reference over ``rows`` [n, S]."""
    from rocmdash.ops.window_excursions import window_excursions_reference

    got = np.asarray(got)
    want = window_excursions_reference(rows, thresholds)
    assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, got.dtype, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)
    return want


def _assert_sorted(got, rows, W, what=""):
    """DeviceWindowSet.export_sorted [S, 1 + W] (count, ascending valid samples, +inf) against
    the oracle's sorted samples - as values: the LDS sort does not order signed zeros."""
    got = np.asarray(got)
    n, S = rows.shape
    assert got.dtype == np.float32 and got.shape == (S, 1 + W), (got.shape, got.dtype)
    ex = _exact.exact_stats(np.ascontiguousarray(rows), PCT)
    for s in range(S):
        nv = int(ex.nv[s])
        assert int(got[s, 0]) == nv, f"{what} series {s}: count {got[s, 0]} != {nv}"
        np.testing.assert_array_equal(got[s, 1:1 + nv], ex.sorted[s], err_msg=f"{what} series {s}")
        assert (got[s, 1 + nv:] == np.inf).all(), f"{what} series {s}: the tail is not +inf"


# ---- a ring's host mirror ---------------------------------------------------------------------
class Mirror:
    """Everything pushed into one ring, oldest first; lost rows are NaN."""

    def __init__(self, width):
        self.rows = np.zeros((0, width), np.float32)
        self.lost = 0

    def push(self, x):
        self.rows = np.concatenate([self.rows, x])

    def lose(self, lo, hi):
        self.rows[lo:hi] = np.nan
        self.lost += hi - lo

    @property
    def head(self):
        return len(self.rows)

    def window(self, W):
        """(the rows a window set holds after a refresh, oldest first; the head)"""
        n = min(self.head, W)
        return self.rows[self.head - n:], self.head


# ---- input columns ----------------------------------------------------------------------------
# quiet NaNs other than numpy's 0x7FC00000: the lost-row fill (all ones), a negative quiet NaN
# without payload, a positive one with a payload. No signalling pattern: the host may quiet it.
ODD_NANS = np.array([0xFFFFFFFF, 0xFFC00000, 0x7FC00001], np.uint32)


def ring_families(first, width):
    """The family of every column of a ring whose first series is ``first``: the ``_exact``
    families in series order (cyclic); a ring of two or more columns ends in ``odd_nan``."""
    fam = [_exact.FAMILIES[(first + c) % len(_exact.FAMILIES)] for c in range(width)]
    if width >= 2:
        fam[-1] = "odd_nan"
    return fam


def ring_rows(rng, families, t0, k, W):
    """[k, width] float32: rows t0 .. t0 + k - 1 of a ring's columns."""
    x = np.empty((k, len(families)), np.float32)
    for c, name in enumerate(families):
        if name == "odd_nan":
            v = rng.normal(100, 20, k).astype(np.float32)
            bad = rng.random(k) < 0.1
            v.view(np.uint32)[bad] = rng.choice(ODD_NANS, int(bad.sum()))
            x[:, c] = v
        else:
            x[:, c] = _exact.family(name, rng, t0, k, W, blips=(3, W + 5))
    return x


# ---- scenarios --------------------------------------------------------------------------------
class nan_rows(int):
    """A step's row count for one ring whose rows are all NaN samples (a source that fails)."""


INVALIDATE = "invalidate"  # a DeviceWindowSet step: invalidate() instead of a push and a refresh


@dataclass(frozen=True)
class Scenario:
    name: str
    kind: str  # "long": LongWindowSet, "device": DeviceWindowSet
    W: int
    widths: tuple
    caps: tuple  # host ring capacities
    steps: tuple  # per refresh: the rows every ring gets (ints / nan_rows), or INVALIDATE
    pinned: bool = True
    pull: bool = True
    use_graph: bool = False

    @property
    def firsts(self):
        return tuple(int(v) for v in np.concatenate([[0], np.cumsum(self.widths)[:-1]]))


def _same_for_all(n, k):
    return (k,) * n


_L84 = ((200, 200), (700, 700), (0, 0), (50, 50), (700, 100), (3, nan_rows(1100)), (40, 60))
_L4 = ((100, 100, 100, 100), (700, 3, 0, 1100), (1, 2, 3, 4), (0, 0, 0, 0), (300, 700, 90, 5), (2, 2, 2, 2))
_DEVICE_WIDTHS = (11, 5, 1, 16, 17, 3, 4, 8, 2, 7)
_MIX = (1, 4, 5, 9, 0, 9, 5, 4, 1, 0)


def _device_steps(W):
    z = _same_for_all
    late = lambda k: z(9, k) + (0,)  # the last ring stays at head 0  # noqa: E731
    return (late(W + 3), _MIX, late(1), z(9, 0) + (5,), z(10, 17), z(10, 257), _MIX[::-1], z(10, 3 * W), INVALIDATE,
            z(10, 2), z(10, 255), z(10, 256), _MIX, (0, 1, 2, 3, 4, 5, 6, 7, 8, 9), z(10, W - 1), _MIX)


def _device(name, W, **kw):
    return Scenario(name, "device", W, _DEVICE_WIDTHS, _same_for_all(10, 8 * W), _device_steps(W), **kw)


SCENARIOS = (
    # LongWindowSet, W = 1024 (the smallest window it accepts): host rings of 256 rows
    Scenario("long_8_4_lost", "long", 1024, (8, 4), (256, 256), _L84),
    Scenario("long_8_4_unpinned", "long", 1024, (8, 4), (256, 256), _L84, pinned=False),
    Scenario("long_13_16_head0", "long", 1024, (13, 16), (256, 512),
             ((300, 0), (800, 0), (0, 600), (5, 7), (0, 0), (900, 33))),
    Scenario("long_1_16_3_12", "long", 1024, (1, 16, 3, 12), (256, 256, 256, 256), _L4),
    Scenario("long_1_16_3_12_graph", "long", 1024, (1, 16, 3, 12), (256, 256, 256, 256), _L4, use_graph=True),
    # the one large case: a lost range across the device wrap
    Scenario("long_65536_wrap", "long", 65536, (8, 4), (4096, 4096), ((61440, 61440), (9000, 100), (50, 50))),
    # DeviceWindowSet: ten rings, three stats launches, two export launches
    _device("device_64_pull", 64),
    _device("device_64_staged", 64, pull=False),
    _device("device_64_unpinned", 64, pinned=False),
    _device("device_512_pull", 512),
    _device("device_512_staged", 512, pull=False),
)
BY_NAME = {sc.name: sc for sc in SCENARIOS}

# csrc/long_window.h, csrc/window_stats.h, csrc/window_stats_rules.h
LW_INGEST_MAX_BYTES = 256 << 10
LW_SEG_COLS = 8
INLINE_ROWS, MAX_INLINE_WIDTH, MAX_RINGS_PER_LAUNCH, MAX_SERIES_PER_LAUNCH, MAX_INCREMENTAL = 4, 16, 4, 256, 256
EXPORT_RINGS_PER_LAUNCH = 8


def _segments(lo, hi, m):
    """Copies of rows [lo, hi) cut at the multiples of m."""
    n = 0
    while lo < hi:
        lo = min(hi, (lo // m + 1) * m)
        n += 1
    return n


def trace_long(sc):
    """What LongWindowSet::stage does with the schedule, from the schedule alone. Per refresh:
    ``rings`` [{added, head, n, lost: (lo, hi), crosses_wrap, all_nan}], ``ingest`` (the small
    refresh staged by the ingest kernel) and ``memcpy`` (DMA copies otherwise)."""
    W, R = sc.W, len(sc.widths)
    head, copied = [0] * R, [0] * R
    nan = [np.zeros(0, bool) for _ in range(R)]  # rows that are NaN whatever the column: lost, or pushed so
    out = []
    for step in sc.steps:
        assert step != INVALIDATE and len(step) == R
        new = [head[i] + int(step[i]) for i in range(R)]
        lows = [max(copied[i], new[i] - W if new[i] > W else 0) for i in range(R)]
        ingest = sc.pinned and all(new[i] - lows[i] <= sc.caps[i] for i in range(R))
        ingest = ingest and 4 * sum((new[i] - lows[i]) * sc.widths[i] for i in range(R)) <= LW_INGEST_MAX_BYTES
        rec = {"rings": [], "ingest": ingest, "memcpy": 0, "rows": sum(int(k) for k in step)}
        for i in range(R):
            h, lo, cap = new[i], lows[i], sc.caps[i]
            nan[i] = np.concatenate([nan[i], np.full(int(step[i]), isinstance(step[i], nan_rows))])
            lost = (0, 0)
            if h - lo > cap:
                lost = (lo, h - cap)
                nan[i][lo:h - cap] = True
                lo = h - cap
            if not ingest:
                rec["memcpy"] += _segments(lo, h, min(W, cap))
            n = min(h, W)
            rec["rings"].append({"added": int(step[i]), "head": h, "n": n, "lost": lost,
                                 "crosses_wrap": lost[1] > lost[0] and lost[0] // W != (lost[1] - 1) // W,
                                 "all_nan": n > 0 and bool(nan[i][h - n:h].all())})
            head[i] = copied[i] = h
        out.append(rec)
    return out


def _incremental(h0, n0, h1, n1, depth, cap):
    """csrc/window_stats_rules.h incremental_step(...).ok"""
    if h1 >= h0 and n0 <= h0:
        s0, s1 = h0 - n0, h1 - n1
        return (s1 >= s0 and h1 - h0 <= MAX_INCREMENTAL and s1 - s0 <= MAX_INCREMENTAL and s0 + depth >= h1
                and n0 <= cap and n1 <= cap)
    return False


def trace_device(sc):
    """What DeviceWindowSet::refresh does with the schedule, from the schedule alone. Per step
    ``{"invalidate": True}`` or ``rings`` [{added, head, n, incremental, inline, pulled, staged,
    wraps}] with the refresh's ``launches``, ``memcpy``, ``pulled_series`` and ``inline_rows``."""
    W, D, R = sc.W, 2 * sc.W, len(sc.widths)
    head, copied, valid, last_head, last_n = [0] * R, [0] * R, [False] * R, [0] * R, [0] * R
    can_pull = sc.pinned and sc.pull
    out = []
    for step in sc.steps:
        if step == INVALIDATE:
            copied, valid = [0] * R, [False] * R
            out.append({"invalidate": True})
            continue
        assert len(step) == R
        rec = {"invalidate": False, "rings": [], "launches": 0, "memcpy": 0, "pulled_series": 0, "inline_rows": 0}
        in_launch = series = 0
        for i in range(R):
            w = sc.widths[i]
            h = head[i] + int(step[i])
            n = min(h, W)
            inc = valid[i] and _incremental(last_head[i], last_n[i], h, n, D, W)
            k_new = h - last_head[i] if inc else 0
            inline = min(k_new, INLINE_ROWS) if inc and w <= MAX_INLINE_WIDTH else 0
            pull = inc and k_new > inline and can_pull
            staged = (not inc) or (k_new > inline and not pull)
            if staged:
                rec["memcpy"] += _segments(max(copied[i], h - D if h > D else 0), h, D)
            if in_launch == MAX_RINGS_PER_LAUNCH or series + w > MAX_SERIES_PER_LAUNCH:
                rec["launches"] += 1
                in_launch = series = 0
            in_launch += 1
            series += w
            rec["pulled_series"] += w if pull else 0
            rec["inline_rows"] += inline
            rec["rings"].append({"added": int(step[i]), "head": h, "n": n, "incremental": inc, "inline": inline,
                                 "pulled": pull, "staged": staged and int(step[i]) > 0, "wraps": h // D})
            head[i] = copied[i] = last_head[i] = h
            valid[i], last_n[i] = True, n
        rec["launches"] += 1
        out.append(rec)
    return out


def trace(sc):
    return trace_long(sc) if sc.kind == "long" else trace_device(sc)


# ---- every export of a set against the references ---------------------------------------------
P, B, L, K = 8, 16, 16, 2
XCORR_CALL = 8  # pairs of one export_xcorr call (rocmdash.ops.window_joint.MAX_PAIRS)
MIN_PERIODS_WINDOW = 512  # rocmdash.ops.window_periods.MIN_SPAN: a set of a shorter window refuses export_periods
_BOUND_FAMILIES = tuple(_bucket_bounds.STATIC)


def export_bounds(S):
    """[S, B]: the uneven families of ``_bucket_bounds``, one after the other by series."""
    return np.stack([_bucket_bounds.STATIC[_BOUND_FAMILIES[s % len(_BOUND_FAMILIES)]](B) for s in range(S)])


def autocorr_span(W):
    """Half the window, so the span cuts it (the smallest span there is at W = 64)."""
    return max(64, W // 2)


def periods_span(W):
    """Half the window where the period trend takes it; from W = 1024 on the autocorrelation's span."""
    return max(MIN_PERIODS_WINDOW, W // 2)


def xcorr_pairs(firsts, widths):
    """``(ring, (a, b))`` for every ring of two or more series, in REVERSED ring order: its first
    series with its last for an even ring index, its last with its first for an odd one."""
    out = []
    for i, (f, w) in enumerate(zip(firsts, widths)):
        if w >= 2:
            out.append((i, (f, f + w - 1) if i % 2 == 0 else (f + w - 1, f)))
    return out[::-1]


class ExportBuffers:
    """The fixed parameters of ``check_all_exports`` on the device and one destination per export,
    for a set of rings of the given widths."""

    def __init__(self, nat, cuda, widths, W, long):
        import torch

        self.nat, self.W, self.long, self.widths = nat, W, long, tuple(widths)
        self.firsts = [int(v) for v in np.concatenate([[0], np.cumsum(widths)[:-1]])]
        S = self.S = int(sum(widths))
        self.bounds = export_bounds(S)
        self.thresholds = np.ascontiguousarray(self.bounds[:, [5, 10]])
        assert self.thresholds.shape == (S, K)
        self.scale = (np.float32(4095.0 / 200.0) * (1 + np.arange(S) % 3)).astype(np.float32)
        self.span = autocorr_span(W)
        # one pair inside each ring of two or more series: its first column with its last
        self.pairs = [(f, f + w - 1) for f, w in zip(self.firsts, widths) if w >= 2]
        self.pair_ring = [i for i, w in enumerate(widths) if w >= 2]
        self.pair_calls = [self.pairs[i:i + 8] for i in range(0, len(self.pairs), 8)]  # at most 8 pairs a call
        # the cross-correlation's pairs: one per such ring too, but listed against the ring order
        self.xpairs = xcorr_pairs(self.firsts, widths)
        self.xpair_calls = [[p for _, p in self.xpairs[i:i + XCORR_CALL]] for i in range(0, len(self.xpairs), XCORR_CALL)]
        self.periods_span = periods_span(W) if W >= MIN_PERIODS_WINDOW else None
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
        self.bd, self.td, self.sd = dev(self.bounds), dev(self.thresholds), dev(self.scale)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=cuda)  # noqa: E731
        self.buckets = new((S, B + 1), torch.float64 if long else torch.float32)
        self.trend = new((S, P + 1, 4), torch.float32)
        self.heatmap = new((S, P + 1, B + 1), torch.int32)
        self.joint = new((max(1, len(self.pairs)), B + 1, B + 1), torch.int32)
        self.quantiles = new((S, P + 1, 4), torch.float32)
        self.autocorr = new((S, L + 1, 4), torch.int64)
        self.excursions = new((S, K, 8), torch.int32)
        self.xcorr = new((max(1, len(self.xpairs)), 2 * L + 1, 6), torch.int64)
        self.periods = None if self.periods_span is None else new((S, P + 1, L + 1, 4), torch.int64)
        self.work_bytes = nat.excursion_workspace_bytes(S, K)
        self.work = new((self.work_bytes,), torch.uint8)
        self.sorted = None if long else new((S, 1 + W), torch.float32)

    def nonfinite_ok(self, ring):
        """Local indices of the ring's series that hold infinities by construction."""
        return tuple(c for c, f in enumerate(ring_families(self.firsts[ring], self.widths[ring])) if f == "inf")


def check_all_exports(ws, mirrors, W, bufs, out, what=""):
    """After a refresh of ``ws`` into ``out`` [S, 8]: every destination filled with -1, all
    nine exports (and export_sorted of a DeviceWindowSet) enqueued, ONE synchronisation, then
    each ring's slice of each output held to that feature's reference over the mirror's window,
    and the cross-checks of the feature tests. export_xcorr takes one pair per ring of two or
    more series, listed in reversed ring order in calls of at most 8 pairs (``xcorr_pairs``).
    export_periods runs only where the set accepts it, W >= 512: the W = 64 scenarios skip it."""
    import torch

    b = bufs
    stream = torch.cuda.current_stream().cuda_stream
    dsts = [b.buckets, b.trend, b.heatmap, b.joint, b.quantiles, b.autocorr, b.excursions]
    for d in dsts + [b.xcorr] + ([] if b.long else [b.sorted]) + ([] if b.periods is None else [b.periods]):
        d.fill_(-1)
    ws.export_buckets(b.bd.data_ptr(), B, b.buckets.data_ptr(), stream)
    ws.export_trend(P, b.trend.data_ptr(), stream)
    ws.export_heatmap(P, b.bd.data_ptr(), B, b.heatmap.data_ptr(), stream)
    at = 0
    for pairs in b.pair_calls:
        ws.export_joint(pairs, b.bd.data_ptr(), B, b.joint[at:].data_ptr(), stream)
        at += len(pairs)
    ws.export_quantiles(P, b.quantiles.data_ptr(), stream, *PCT)
    ws.export_autocorr(b.span, b.sd.data_ptr(), L, b.autocorr.data_ptr(), stream)
    ws.export_excursions(b.td.data_ptr(), K, b.excursions.data_ptr(), b.work.data_ptr(), b.work_bytes, stream)
    at = 0
    for pairs in b.xpair_calls:
        ws.export_xcorr(pairs, b.span, b.sd.data_ptr(), L, b.xcorr[at:].data_ptr(), stream)
        at += len(pairs)
    if b.periods is not None:
        ws.export_periods(b.periods_span, P, b.sd.data_ptr(), L, b.periods.data_ptr(), stream)
    if not b.long:
        ws.export_sorted(b.sorted.data_ptr(), stream)
    torch.cuda.synchronize()
    xcorr = b.xcorr.cpu().numpy()
    periods = None if b.periods is None else b.periods.cpu().numpy()
    xslot = {ring: k for k, (ring, _) in enumerate(b.xpairs)}
    buckets, trend, heatmap, joint, quantiles, autocorr, excursions = (d.cpu().numpy() for d in dsts)
    stats = out.cpu().numpy()
    sorted_ = None if b.long else b.sorted.cpu().numpy()

    for i, (m, f, w) in enumerate(zip(mirrors, b.firsts, b.widths)):
        rows, head = m.window(W)
        sl = slice(f, f + w)
        at = f"{what} ring {i} (series {f} .. {f + w - 1}, head {head})"
        (_assert_long_counts if b.long else _assert_counts)(buckets[sl], rows.T, b.bounds[sl], what=f"{at} buckets")
        _assert_trend(trend[sl], rows, head, W, P, what=f"{at} trend")
        _assert_heatmap(heatmap[sl], rows, head, W, P, b.bounds[sl], what=f"{at} heatmap")
        _assert_quantiles(quantiles[sl], rows, head, W, P, PCT, b.nonfinite_ok(i), what=f"{at} quantiles")
        _assert_autocorr(autocorr[sl], rows.T, b.scale[sl], L, b.span, what=f"{at} autocorr")
        _assert_excursions(excursions[sl], rows, b.thresholds[sl], what=f"{at} excursions")
        if i in b.pair_ring:
            k = b.pair_ring.index(i)
            _assert_joint(joint[k:k + 1], rows, [(0, w - 1)], b.bounds[sl], what=f"{at} joint")
        if i in xslot:
            k = xslot[i]
            pa, pb = b.xpairs[k][1]
            _window_xcorr.assert_xcorr(xcorr[k:k + 1], rows.T, [(pa - f, pb - f)], b.scale[sl], L, b.span,
                                       what=f"{at} xcorr slot {k} pair ({pa}, {pb})")
            if head == 0:
                assert not xcorr[k].any(), f"{at} xcorr slot {k}: a ring without rows"
        if periods is not None:
            _assert_periods(periods[sl], rows, b.scale[sl], head, W, P, L, b.periods_span, what=f"{at} periods")
        if sorted_ is not None:
            _assert_sorted(sorted_[sl], rows, W, what=f"{at} sorted")
    # the exports against each other and against the statistics of the same refresh
    np.testing.assert_array_equal(heatmap.sum(axis=2), trend[:, :, 3], err_msg=f"{what}: heatmap bins / trend counts")
    np.testing.assert_array_equal(np.cumsum(heatmap.sum(axis=1), axis=1).astype(buckets.dtype), buckets,
                                  err_msg=f"{what}: heatmap slots / buckets")
    np.testing.assert_array_equal(trend[:, :, 3].sum(axis=1), stats[:, _exact.COUNT], err_msg=f"{what}: trend counts / count")
    np.testing.assert_array_equal(quantiles[:, :, 3], trend[:, :, 3], err_msg=f"{what}: quantile counts / trend counts")
    np.testing.assert_array_equal(excursions[:, 0, 1], stats[:, _exact.COUNT], err_msg=f"{what}: excursions' valid / count")
    if periods is not None and b.periods_span == b.span:  # the slots cut the autocorrelation's rows: lag 0 adds up
        np.testing.assert_array_equal(periods[:, :, 0, 0].sum(axis=1), autocorr[:, 0, 0], err_msg=f"{what}: periods' n_0 / autocorr")
        np.testing.assert_array_equal(periods[:, :, 0, 3].sum(axis=1), autocorr[:, 0, 3], err_msg=f"{what}: periods' Sxy_0 / autocorr")
