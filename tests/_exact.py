"""The exact oracle of the window statistics: which fp32 value every output must be.

Every statistic but the mean is a selection - min, max, last, count and the six order
statistics behind the three percentiles - and the kernels' output arithmetic
(``wanted_positions`` / ``percentile_between`` in csrc/window_stats_rules.h, ``lw_positions``
in csrc/long_window_dev.h, the tail of the last scan in csrc/long_window_radix.hip and
``node_select_kernel`` in csrc/node_window.hip) is small and deterministic, 0-based:

    p    = double(float(pct)) / 100 * (nv - 1)
    lo   = floor(p);  hi = min(lo + 1, nv - 1)
    frac = double(float(p - lo))
    out  = float(frac >= 0.5 ? x1 - (x1 - x0) * (1 - frac) : x0 + (x1 - x0) * frac)

``exact_stats`` repeats it in numpy over the valid fp32 samples sorted by the kernels' key
order; ``assert_exact`` holds an output to it: equality wherever no arithmetic can move the
value, one fp32 ulp (and inside [x0, x1]) where the kernel interpolates, and a derived
bound on the mean. Plain numpy, no GPU and no native code; imported like ``_golden``.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MIN, MAX, MEAN, P0, LAST, COUNT = 0, 1, 2, 3, 6, 7
NUM_STATS = 8


def fkey(x) -> np.ndarray:
    """Order-preserving float32 -> uint32 key on the IEEE bit pattern (csrc/long_window_dev.h
    ``fkey``): -0.0 sorts before +0.0."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def kfloat(k) -> np.ndarray:
    k = np.ascontiguousarray(k, np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(np.float32)


def positions(nv, pct):
    """([lo0, hi0, lo1, hi1, lo2, hi2], float32 frac[3]) of the percentiles over ``nv`` valid
    samples, by the kernels' arithmetic."""
    last = int(nv) - 1 if nv else 0
    pos, frac = [], []
    for q in pct:
        p = float(np.float32(q)) / 100.0 * float(last)
        lo = min(int(np.floor(p)), last)
        pos += [lo, lo + 1 if lo + 1 < nv else last]
        frac.append(np.float32(p - float(lo)))
    return pos, np.array(frac, np.float32)


def percentile_between(x0, x1, frac) -> np.ndarray:
    """The kernels' interpolation in numpy float64, rounded to float32."""
    x0, x1 = np.asarray(x0, np.float64), np.asarray(x1, np.float64)
    f = np.asarray(frac, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(f >= 0.5, x1 - (x1 - x0) * (1.0 - f), x0 + (x1 - x0) * f).astype(np.float32)


@dataclass
class Exact:
    pct: tuple
    sorted: list  # per series: the valid fp32 samples in key order
    nv: np.ndarray  # [S]
    pos: np.ndarray  # [S, 6]
    frac: np.ndarray  # [S, 3] float32
    min: np.ndarray  # [S] float32 (NaN: no valid sample)
    max: np.ndarray
    last: np.ndarray  # [S] float32: the raw newest sample
    count: np.ndarray  # [S]
    x0: np.ndarray  # [S, 3] float32
    x1: np.ndarray
    percentile: np.ndarray  # [S, 3] float32
    mean: np.ndarray  # [S] float64
    mean_abs: np.ndarray  # [S] float64: the mean of |x|

    def output(self) -> np.ndarray:
        """The [S, 8] float32 output the oracle expects (mean rounded to float32)."""
        S = len(self.nv)
        out = np.full((S, NUM_STATS), np.nan, np.float32)
        out[:, MIN], out[:, MAX] = self.min, self.max
        with np.errstate(over="ignore", invalid="ignore"):
            out[:, MEAN] = self.mean.astype(np.float32)
        out[:, P0:P0 + 3] = self.percentile
        out[:, LAST], out[:, COUNT] = self.last, self.count
        return out


def exact_stats(rows, pct) -> Exact:
    """``rows``: [n, S] float32, oldest first."""
    rows = np.asarray(rows)
    assert rows.ndim == 2 and rows.dtype == np.float32, (rows.shape, rows.dtype)
    n, S = rows.shape
    valid = ~np.isnan(rows)
    nv = valid.sum(axis=0).astype(np.int64)
    keys = fkey(rows).reshape(n, S)
    keys[~valid] = np.uint32(0xFFFFFFFF)  # a NaN's own pattern: no valid sample keys to it
    keys = np.sort(keys, axis=0)
    nan32 = np.float32(np.nan)
    ex = Exact(pct=tuple(float(p) for p in pct), sorted=[], nv=nv, pos=np.zeros((S, 6), np.int64),
               frac=np.zeros((S, 3), np.float32), min=np.full(S, nan32), max=np.full(S, nan32),
               last=rows[-1].copy() if n else np.full(S, nan32), count=nv.copy(), x0=np.full((S, 3), nan32),
               x1=np.full((S, 3), nan32), percentile=np.full((S, 3), nan32), mean=np.full(S, np.nan),
               mean_abs=np.full(S, np.nan))
    for s in range(S):
        v = kfloat(keys[:nv[s], s])
        ex.sorted.append(v)
        pos, frac = positions(nv[s], ex.pct)
        ex.pos[s], ex.frac[s] = pos, frac
        if not nv[s]:
            continue
        ex.min[s], ex.max[s] = v[0], v[-1]
        ex.x0[s], ex.x1[s] = v[pos[0::2]], v[pos[1::2]]
        # extended precision: the reference's own error stays far below the bound's terms
        with np.errstate(over="ignore", invalid="ignore"):
            w = v.astype(np.longdouble)
            ex.mean[s] = float(w.sum() / nv[s])
            ex.mean_abs[s] = float(np.abs(w).sum() / nv[s])
    ex.percentile = percentile_between(ex.x0, ex.x1, ex.frac)
    return ex


def _same(got, want) -> bool:
    """Equal as values: NaN where the oracle has NaN, -0.0 == +0.0."""
    return bool(np.isnan(got)) if np.isnan(want) else bool(got == want)


def _within_one_ulp(got: np.float32, want: np.float32) -> bool:
    with np.errstate(over="ignore"):
        return bool(got == want or got == np.nextafter(want, np.float32(-np.inf))
                    or got == np.nextafter(want, np.float32(np.inf)))


def ulp32(x) -> float:
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.spacing(np.abs(np.float32(x))))


def mean_bound(ex: Exact, s: int, sum_group: int) -> float:
    """|got - mean64| allowed for series ``s``: fp32 rounding inside the kernel's runs of
    ``sum_group`` fp32 adds, fp64 rounding of the nv adds, the final rounding to float32."""
    return ((sum_group - 1) * 2.0 ** -24 + float(ex.nv[s]) * 2.0 ** -53) * float(ex.mean_abs[s]) + ulp32(ex.mean[s])


def assert_exact(got, rows, pct, *, sum_group, last=True, skip_nonfinite=()) -> int:
    """Hold ``got`` [S, 8] to the oracle over ``rows`` ([n, S] float32, or the ``Exact`` that
    ``exact_stats`` made of them with the same ``pct``). Returns the number of individual
    output comparisons made."""
    ex = rows if isinstance(rows, Exact) else exact_stats(rows, pct)
    assert ex.pct == tuple(float(p) for p in pct), (ex.pct, pct)
    assert int(sum_group) >= 1
    got = np.asarray(got)
    S = len(ex.nv)
    assert got.shape == (S, NUM_STATS), (got.shape, S)
    g32 = got.astype(np.float32)
    assert np.array_equal(g32.astype(np.float64), got.astype(np.float64), equal_nan=True), "outputs are fp32 values"
    skip = set(int(s) for s in skip_nonfinite)
    assert all(0 <= s < S for s in skip), (skip, S)
    n = 0
    for s in range(S):
        g = g32[s]
        where = f"series {s} (nv {ex.nv[s]}, pct {ex.pct})"
        assert g[COUNT] == ex.count[s], f"{where}: count {g[COUNT]} != {ex.count[s]}"
        n += 1
        if last:
            assert _same(g[LAST], ex.last[s]), f"{where}: last {g[LAST]!r} != {ex.last[s]!r}"
            n += 1
        if not ex.nv[s]:
            for c in range(6):
                assert np.isnan(g[c]), f"{where}: column {c} is {g[c]!r} with no valid sample"
                n += 1
            continue
        assert _same(g[MIN], ex.min[s]), f"{where}: min {g[MIN]!r} != {ex.min[s]!r}"
        assert _same(g[MAX], ex.max[s]), f"{where}: max {g[MAX]!r} != {ex.max[s]!r}"
        n += 2
        if s in skip and not (np.all(np.isfinite(ex.x0[s])) and np.all(np.isfinite(ex.x1[s]))
                              and np.isfinite(ex.mean[s]) and np.isfinite(ex.mean_abs[s])):
            continue
        for q in range(3):
            x0, x1, f, want, have = ex.x0[s, q], ex.x1[s, q], ex.frac[s, q], ex.percentile[s, q], g[P0 + q]
            what = (f"{where}: p{ex.pct[q]:g} = {have!r}, oracle {want!r} (x0 {x0!r} at {ex.pos[s, 2 * q]}, "
                    f"x1 {x1!r} at {ex.pos[s, 2 * q + 1]}, frac {f!r})")
            if f == 0 or x0 == x1:  # no arithmetic can move it: the order statistic itself
                assert _same(have, x0), what
            else:
                assert _within_one_ulp(have, want), what
                assert x0 <= have <= x1, what + ": outside [x0, x1]"
            n += 1
        bound = mean_bound(ex, s, int(sum_group))
        err = abs(float(g[MEAN]) - float(ex.mean[s]))
        assert err <= bound, f"{where}: mean {g[MEAN]!r} vs {ex.mean[s]!r}: |diff| {err:.3e} > {bound:.3e}"
        n += 1
    return n


def expected_comparisons(S: int, *, last=True, skipped=0) -> int:
    """What ``assert_exact`` returns for ``S`` series of which ``skipped`` had their
    percentile and mean checks skipped: count, last, then min, max, three percentiles and
    the mean (or six NaNs with no valid sample)."""
    per = NUM_STATS if last else NUM_STATS - 1
    return S * per - 4 * skipped


# ---- input families of the exact-rank tests ---------------------------------------------
# One column each (float32), as a function of the absolute row index t, so that a test can
# push the same series in pieces: the places where a selection goes wrong.
ZEROES = np.array([-0.0, 0.0, 1.4e-45, -1.4e-45, 1e-40, -1e-40, 1.5, -1.5], np.float32)
FAMILIES = ("narrow", "narrow_nan", "wide", "wide_nan", "zeroes", "boundary", "ties", "ties_nan", "ramp_up",
            "ramp_down", "sparse1", "sparse2", "sparse3", "blip", "inf",
            # the columns past the first fifteen (wider rings)
            "all_nan", "constant", "normal", "normal_nan", "narrow_negative", "denormal")
INF_SERIES = FAMILIES.index("inf")  # the one series a test may put in skip_nonfinite
CONTINUOUS = ("narrow", "wide", "normal", "ramp_up", "inf")


def family(name: str, rng, t0: int, k: int, W: int, blips=()) -> np.ndarray:
    """Rows t0 .. t0 + k - 1 of one family, for windows of W rows."""
    t = np.arange(t0, t0 + k, dtype=np.int64)

    def holes(x):
        x = x.astype(np.float32)
        x[rng.random(k) < 0.03] = np.nan
        return x

    def sparse(j):  # about j valid samples in any W consecutive rows
        period = max(1, W // j)
        return np.where(t % period == 7 % period, rng.normal(50, 10, k), np.nan)

    if name in ("narrow", "narrow_nan"):  # adjacent order statistics a few ulp apart
        x = rng.normal(100, 0.01, k)
        return holes(x) if name.endswith("_nan") else x.astype(np.float32)
    if name in ("wide", "wide_nan"):  # mixed sign, every exponent: every radix digit
        x = rng.normal(0, 1, k) * 10.0 ** rng.uniform(-30, 30, k)
        return holes(x) if name.endswith("_nan") else x.astype(np.float32)
    if name == "zeroes":  # signed zeros and denormals
        return rng.choice(ZEROES, k)
    if name == "boundary":  # half 16.0, half 17.0: p50 straddles a tie boundary
        return np.where(t % 2 == 0, 16.0, 17.0).astype(np.float32)
    if name in ("ties", "ties_nan"):
        x = rng.integers(0, 6, k)
        return holes(x) if name.endswith("_nan") else x.astype(np.float32)
    if name == "ramp_up":  # every row the new max
        return t.astype(np.float32)
    if name == "ramp_down":  # every row the new min
        return (-t).astype(np.float32)
    if name.startswith("sparse"):
        return sparse(int(name[-1])).astype(np.float32)
    if name == "blip":  # all NaN but the rows in `blips`: nv goes 0, 1, 0
        return np.where(np.isin(t, np.asarray(list(blips), np.int64)), 3.5, np.nan).astype(np.float32)
    if name == "inf":
        x = rng.normal(0, 1, k).astype(np.float32)
        u = rng.random(k)
        x[u < 0.005] = np.inf
        x[u > 0.995] = -np.inf
        return x
    if name == "all_nan":
        return np.full(k, np.nan, np.float32)
    if name == "constant":
        return np.full(k, 42.0, np.float32)
    if name in ("normal", "normal_nan"):
        x = rng.normal(100, 20, k)
        return holes(x) if name.endswith("_nan") else x.astype(np.float32)
    if name == "narrow_negative":
        return rng.normal(-100, 0.01, k).astype(np.float32)
    if name == "denormal":
        return (rng.normal(0, 1, k) * 1e-40).astype(np.float32)
    raise KeyError(name)


def family_rows(rng, t0: int, k: int, W: int, width: int = 15, first: int = 0, blips=()) -> np.ndarray:
    """[k, width] rows t0 .. t0 + k - 1 of families first .. first + width - 1."""
    x = np.empty((k, width), np.float32)
    for c in range(width):
        x[:, c] = family(FAMILIES[first + c], rng, t0, k, W, blips)
    return x


def long_window_sum_group() -> int:
    """The longest run of terms the long-window passes add in fp32: the largest value of the
    ``UG`` template default in csrc/long_window_pass.h."""
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "long_window_pass.h")
    with open(path) as f:
        m = re.search(r"int UG = \(WM <= \d+ \? (\d+) : (\d+)\)", f.read())
    assert m, "csrc/long_window_pass.h: the UG template default moved"
    return max(int(m.group(1)), int(m.group(2)))
