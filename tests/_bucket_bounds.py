"""Bounds and samples that make the kernels that bin by the le rule WALK. Three kernels hold a
private copy of it - the streaming le-bucket kernel (csrc/long_window_buckets.hip), the window
heatmap (csrc/window_heatmap.hip) and the joint histogram (csrc/window_joint.hip): a lane that
left its bin guesses the new one as if its bounds were evenly spaced,

    g = clamp(ceil((x - b[0]) * (B - 1) / (b[B-1] - b[0])), 0, B)        (NaN -> 0)

and then steps edge by edge to the bin that holds the sample. On evenly spaced bounds the
walk is at most one step; the families here are finite, strictly ascending and uneven, so
that the guess is far off - below, above, or no guess at all (the span overflows, the inverse
is inf) - and the walk is what the counts depend on. ``guess_distance`` is a model of the
guess alone, for preconditions ("these inputs need the walk"); it is never an expected value:
those come from the references of ``rocmdash.ops.window_buckets``, ``window_heatmap`` and
``window_joint``.

What the three kernels' tests share is here too: the launch schedule after which every bounds
family has met every sample family (``_shifts``), the windows of a ring (``_windows``), a
ring's columns (``_ring_inputs``), the walk precondition over a window's own samples
(``_walkers``) and NaN put into a column after its bounds were derived (``with_nans``).

Also the bounds the sorted-window tests use (``bounds_row``: on samples / one ulp beside
them) and their input rows (``one_shot_rows``). Plain numpy, no GPU and no native code;
imported like ``_exact``.
"""

from __future__ import annotations

import numpy as np

import _exact

F32 = np.float32
INF = F32(np.inf)


# ---- bounds --------------------------------------------------------------------------------
def geometric(B: int) -> np.ndarray:
    """0.005 * 2^k, the Prometheus style: dense at the low end, the guess falls too low."""
    return (0.005 * 2.0 ** np.arange(B)).astype(F32)


def geometric_down(B: int) -> np.ndarray:
    """The mirror image: -0.005 * 2^k descending in k, dense at the top end, the guess too high."""
    return np.ascontiguousarray(-geometric(B)[::-1])


def huge_span(B: int) -> np.ndarray:
    """Linear from -3e38 to 3e38: ``b[B-1] - b[0]`` overflows, bins per unit is 0, every guess 0."""
    return np.linspace(-3e38, 3e38, B).astype(F32) if B > 1 else np.array([-3e38], F32)


def denormal(B: int) -> np.ndarray:
    """Integer multiples of 2^-149 around 0, 0.0 among them: bins per unit overflows to inf."""
    return ((np.arange(B) - B // 2) * 2.0 ** -149).astype(F32)


def ulp_run(B: int, start: float = 1.0) -> np.ndarray:
    """B consecutive floats from ``start`` (positive) up."""
    first = int(np.array([start], F32).view(np.int32)[0])
    assert first > 0
    return (first + np.arange(B, dtype=np.int32)).astype(np.int32).view(F32)


def clustered(B: int) -> np.ndarray:
    """-1e30, consecutive floats from 1.0, 1e30: every guess lands in the middle of the span."""
    if B < 3:
        return np.array([-1e30, 1e30][:B] if B == 2 else [1.0], F32)
    return np.concatenate([[F32(-1e30)], ulp_run(B - 2, 1.0), [F32(1e30)]]).astype(F32)


def bounds_row(v, B: int, kind: str) -> np.ndarray:
    """B finite, strictly ascending fp32 bounds for one series from its valid samples ``v``:
    ``on_samples`` = every k-th distinct sorted sample itself; ``between`` = one ulp above or
    below such a sample (alternating): between its neighbours where they are a few ulp apart.
    Series with fewer than B distinct finite samples get further bounds one ulp apart above
    the last (or around 0 with no sample at all)."""
    f32 = np.float32
    c = np.unique(v[np.isfinite(v)]).astype(f32)  # ascending, -0.0 == +0.0 merged
    if len(c):
        c = c[np.unique(np.linspace(0, len(c) - 1, min(B, len(c))).astype(np.int64))]
        if kind == "between":
            toward = np.where(np.arange(len(c)) % 2 == 0, f32(np.inf), f32(-np.inf)).astype(f32)
            c = np.unique(np.nextafter(c, toward).astype(f32))
            c = c[np.isfinite(c)]
    out = [f32(x) for x in c]
    if not out:
        out = [f32(-1e-45)]
    while len(out) < B:
        out.append(np.nextafter(out[-1], f32(np.inf)).astype(f32))
    out = np.array(out[:B], f32)
    assert np.isfinite(out).all() and (np.diff(out) > 0).all()
    return out


STATIC = {"geometric": geometric, "geometric_down": geometric_down, "huge_span": huge_span, "denormal": denormal,
          "ulp_run": ulp_run, "clustered": clustered}
FROM_SAMPLES = ("on_samples", "between")
BOUNDS = tuple(STATIC) + FROM_SAMPLES
# the least walk, in bins, the family must ask of the kernel on samples that visit every bin
# (B >= 16), and its direction: +1 up (the guess too low), -1 down, 0 either. A quarter of
# what the fp32 model finds (55 up, 56 down, 62 and 31 of B = 63): the GPU may round the
# guess another way (contraction, its division), by a bin or two, not by three quarters.
WALKS = {"geometric": (lambda B: B // 4, +1), "geometric_down": (lambda B: B // 4, -1),
         "huge_span": (lambda B: B - 1, +1), "denormal": (lambda B: B // 4, 0), "clustered": (lambda B: B // 4, 0)}


def bounds_for(name: str, B: int, v=None) -> np.ndarray:
    """Family ``name``'s bounds; ``on_samples`` / ``between`` from the samples ``v``."""
    if name in STATIC:
        return STATIC[name](B)
    return bounds_row(np.asarray(v, F32)[~np.isnan(v)], B, name)


def guess_distance(x, b) -> np.ndarray:
    """int64 per sample: bins from the kernel's guess to the sample's bin
    ``searchsorted(b, x, "left")`` - positive: the walk goes up (the guess was too low),
    negative: down. The guess in fp32 as the kernel writes it, its clamp and NaN -> 0
    included; 0 for a NaN sample (the kernel skips it)."""
    x, b = np.asarray(x, F32), np.asarray(b, F32)
    B = len(b)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        inv = F32(B - 1) / F32(b[-1] - b[0]) if B > 1 else F32(0)
        g = np.ceil(((x - b[0]).astype(F32) * inv).astype(F32))
    g = np.where(np.isnan(g), F32(0), g)  # fmaxf(NaN, 0) = 0
    g = np.minimum(np.maximum(g, F32(0)), F32(B)).astype(np.int64)
    d = np.searchsorted(b, x, side="left").astype(np.int64) - g
    return np.where(np.isnan(x), 0, d)


def walk_reached(x, b) -> tuple:
    """(the longest walk up, the longest walk down) over the samples ``x``, in bins."""
    d = guess_distance(x, b)
    return (int(max(d.max(), 0)), int(max(-d.min(), 0))) if d.size else (0, 0)


def walks_enough(name: str, x, b) -> bool:
    """The precondition of a walking family on the samples a test really uses."""
    least, direction = WALKS[name]
    up, down = walk_reached(x, b)
    need = least(len(b))
    return {+1: up >= need, -1: down >= need, 0: max(up, down) >= need}[direction]


# ---- samples -------------------------------------------------------------------------------
def hop(rng, n: int, b) -> np.ndarray:
    """-inf, +inf, b[0], b[-1], then a sample on or one ulp above a random bound of the
    inner bins, and again: every sample leaves the bin of the one before (B >= 4)."""
    b = np.asarray(b, F32)
    B = len(b)
    k = rng.integers(1, B - 2, n) if B >= 4 else rng.integers(0, B, n)  # B >= 4: bins 1 .. B - 2
    far = np.where(rng.random(n) < 0.5, b[k], np.nextafter(b[k], INF)).astype(F32)
    x = np.empty(n, F32)
    i = np.arange(n)
    for r, v in enumerate((-INF, INF, b[0], b[-1])):
        x[i % 5 == r] = v
    x[i % 5 == 4] = far[i % 5 == 4]
    return x


def stairs(rng, n: int, b) -> np.ndarray:
    """One sample per bound, up on the bounds themselves, then down one ulp above them."""
    b = np.asarray(b, F32)
    cycle = np.concatenate([b, np.nextafter(b, INF)[::-1]]).astype(F32)
    return np.tile(cycle, n // len(cycle) + 1)[:n].copy()


def beside(rng, n: int, b) -> np.ndarray:
    """b[k] itself and its two neighbours among the floats, for random k."""
    b = np.asarray(b, F32)
    k, u = rng.integers(0, len(b), n), rng.integers(0, 3, n)
    return np.where(u == 0, np.nextafter(b[k], -INF), np.where(u == 1, b[k], np.nextafter(b[k], INF))).astype(F32)


def runs(rng, n: int, b) -> np.ndarray:
    """Runs of 5 to 200 samples inside one random bin (lo, hi], alternating between its two
    ends - one ulp above lo, and hi itself - then a jump to another bin."""
    b = np.asarray(b, F32)
    B = len(b)
    low = np.concatenate([[np.nextafter(b[0], -INF)], np.nextafter(b, INF)]).astype(F32)  # bin k's lowest float
    high = np.concatenate([b, [np.nextafter(np.nextafter(b[-1], INF), INF)]]).astype(F32)  # ... and highest
    x = np.empty(n, F32)
    at = 0
    while at < n:
        k, length = int(rng.integers(0, B + 1)), int(rng.integers(5, 201))
        seg = np.where(np.arange(length) % 3 == 1, low[k], high[k])
        x[at:at + length] = seg[:n - at]
        at += length
    assert np.isfinite(x).all()
    return x


def zeroes(rng, n: int, b) -> np.ndarray:
    return np.where(rng.random(n) < 0.5, F32(0.0), F32(-0.0)).astype(F32)


SAMPLES = {"hop": hop, "stairs": stairs, "beside": beside, "runs": runs, "zeroes": zeroes}
SAMPLE_KINDS = tuple(SAMPLES) + ("exact",)  # exact: a column of _exact.FAMILIES
VISIT_EVERY_BIN = ("hop", "stairs", "beside")  # on these a walking family must show its walk


def exact_column(rng, j: int, n: int) -> np.ndarray:
    """Column ``j`` (cyclic) of the ``_exact`` families, n rows of a window of n."""
    return _exact.family(_exact.FAMILIES[j % len(_exact.FAMILIES)], rng, 0, n, n, blips=(n // 2,))


def column(rng, bounds_name: str, sample_kind: str, j: int, n: int, B: int) -> tuple:
    """(bounds [B], samples [n]) of one series: the bounds of ``on_samples`` / ``between`` come
    from column j of the ``_exact`` families, which is also what the ``exact`` samples are."""
    v = exact_column(rng, j, n)
    b = bounds_for(bounds_name, B, v)
    x = v if sample_kind == "exact" else SAMPLES[sample_kind](rng, n, b)
    return b, np.ascontiguousarray(x, F32)


# ---- rings: what the tests of the three kernels launch ---------------------------------------
F, NS = len(BOUNDS), len(SAMPLE_KINDS)
UNREAD = np.float32(1.0)  # what the columns >= cols hold: a bound of ulp_run and clustered, a count for any


def _shifts(cols):
    """(offset, shift): column c takes bounds family (c + offset) % F and sample family
    (c + shift) % NS. The fewest launches, in order, after which every bounds family has met
    every sample family in some column."""
    seen, keep = set(), []
    for o in range(F):
        for s in range(NS):
            pairs = {((c + o) % F, (c + s) % NS) for c in range(cols)}
            if not pairs <= seen:
                seen |= pairs
                keep.append((o, s))
    assert len(seen) == F * NS
    return keep


def _windows(depth):
    """(kind, head, n): one row; part-filled, unwrapped; the full ring as two blocks; a
    part-filled window that wraps, at a head past 2^32."""
    part = depth // 2 + 3
    w = [("n = 1", depth + 7, 1), ("part, unwrapped", part, part), ("full, two blocks", 2 * depth + depth // 3 + 1, depth),
         ("wrapped, head > 2^32", (1 << 32) + 12345, part)]
    first = [(head - n) & (depth - 1) for _, head, n in w]
    assert first[1] == 0 and first[2] > 0 and first[3] + part > depth and w[3][1] - part > 1 << 32
    return w


def _ring_inputs(depth, stride, cols, B, o, s):
    """(rows [depth, stride], bounds [cols, B], names per column): every row holds samples (a
    window that is not full leaves rows that would count outside it)."""
    rng = np.random.default_rng(1000 * depth + 100 * stride + 10 * B + 7 * o + s)
    rows = np.full((depth, stride), UNREAD, np.float32)
    bounds = np.empty((cols, B), np.float32)
    names = []
    for c in range(cols):
        names.append((BOUNDS[(c + o) % F], SAMPLE_KINDS[(c + s) % NS]))
        bounds[c], rows[:, c] = column(rng, names[c][0], names[c][1], c + o, depth, B)
    return rows, bounds, names


def _walkers(rows, bounds, names, head, n):
    """The walking families among the columns whose samples visit every bin, each held to its
    precondition over the window's own samples."""
    depth = rows.shape[0]
    slots = np.arange(head - n, head, dtype=np.int64) & (depth - 1)
    found = set()
    for c, (family, kind) in enumerate(names):
        if family in WALKS and kind in VISIT_EVERY_BIN:
            x = rows[slots, c]
            assert walks_enough(family, x, bounds[c]), (c, family, kind, walk_reached(x, bounds[c]))
            found.add(family)
    return found


def with_nans(rng, x, share) -> np.ndarray:
    """A copy of the column ``x`` with about ``share`` of its samples replaced by NaN - after the
    column's bounds were derived, so they stay what they were. NaN only removes samples: a walk
    precondition is computed on the column before this."""
    x = np.array(x, F32)
    x[rng.random(len(x)) < share] = np.nan
    return x


# The rings of the heatmap's and the joint histogram's one-shot tests (test_gpu_window_heatmap_bounds.py,
# test_gpu_window_joint_bounds.py; test_bucket_bounds_walks.py holds their inputs to the walk
# preconditions without a GPU). Heatmap: (depth, stride, cols, P, rows_per_col), the window P x
# rows_per_col = depth; one wave streams a slot of stride x rows_per_col <= 2048 floats, eight waves a larger one.
HEATMAP_RINGS = [(1024, 1, 1, 8, 128), (1024, 3, 3, 8, 128), (1024, 12, 7, 8, 128), (1024, 13, 13, 64, 16),
                 (1024, 23, 23, 8, 128), (4096, 64, 64, 8, 512)]
HEATMAP_B = [1, 2, 3, 16, 63]
JOINT_RINGS = [(1024, 2, 2), (1024, 5, 5), (1024, 7, 7), (1024, 12, 7), (1024, 23, 23), (4096, 64, 64)]
JOINT_B = [1, 2, 3, 16, 31]
NAN_SHARE = 0.05


def _launch_inputs(depth, stride, cols, B, i, o, s):
    """Launch ``i`` of a ring's schedule ``_shifts(cols)[i] == (o, s)``: (the rows of
    ``_ring_inputs``, the rows the kernel gets, bounds, names). In every second launch the
    kernel's rows have NaN in NAN_SHARE of every column that is not ``exact`` (those hold the
    NaN of their own families)."""
    clean, bounds, names = _ring_inputs(depth, stride, cols, B, o, s)
    rows = clean.copy()
    if i % 2:
        rng = np.random.default_rng(31 * depth + 17 * stride + 5 * B + i)
        for c, (_, kind) in enumerate(names):
            if kind != "exact":
                rows[:, c] = with_nans(rng, clean[:, c], NAN_SHARE)
    return clean, rows, bounds, names


# ---- window sets: what the export tests of the heatmap and the joint histogram refresh -----------
EXPORT_KINDS = ("on_samples", "between", "geometric", "huge_span")  # by series, as the long buckets' export test
EXPORT_WIDTHS = (8, 13)  # LongWindowSet: two segments, unaligned rows


def export_steps(W):
    """Rows pushed before each refresh: a part-filled window, a full one, +1 row, none, +100,
    +257 and enough to wrap the device ring (W rows of a LongWindowSet, 2 W of a DeviceWindowSet)."""
    return [W // 2 + 5, W // 2 + 32, 1, 0, 100, 257, W + W // 4 + 7]


class ExportRings:
    """Two rings of 8 and 13 series fed the 21 ``_exact`` families, in a LongWindowSet
    (``long``) or a DeviceWindowSet of window W, with everything pushed kept oldest first."""

    def __init__(self, nat, W, long, seed):
        nat.set_pinned_host_rings(True)
        if not long:
            nat.set_pull_mode(True)
        self.W, self.S = W, sum(EXPORT_WIDTHS)
        self.rings = [nat.SeriesRing(w, 2 * W if long else 8 * W) for w in EXPORT_WIDTHS]
        self.ws = nat.LongWindowSet(W, 0) if long else nat.DeviceWindowSet(W, 0)
        for r in self.rings:
            self.ws.add_ring(r)
        self.rows = np.zeros((0, self.S), F32)
        self.rng = np.random.default_rng(seed)
        self.t = 0

    def push(self, k):
        if not k:
            return
        x = _exact.family_rows(self.rng, self.t, k, self.W, width=self.S, blips=(5, self.W + 8))
        ts = np.arange(self.t + 1, self.t + 1 + k, dtype=np.uint64)
        c0 = 0
        for r, w in zip(self.rings, EXPORT_WIDTHS):
            r.push_many(np.ascontiguousarray(x[:, c0:c0 + w]), ts)
            c0 += w
        self.rows = np.concatenate([self.rows, x])
        self.t += k

    def window(self):
        """[n, S]: the rows the set holds after a refresh, oldest first (head = ``t``)."""
        return self.rows[-self.W:]

    def bounds(self, B):
        """[S, B]: EXPORT_KINDS by series, the two from-samples kinds from this very window."""
        x = self.window()
        return np.stack([bounds_for(EXPORT_KINDS[s % len(EXPORT_KINDS)], B, x[:, s]) for s in range(self.S)])


_ROWS = {}


def one_shot_rows(n: int) -> np.ndarray:
    """[S, n], read-only: the 21 families, + a constant run, + one series with -inf and +inf
    at its ends."""
    if n not in _ROWS:
        rng = np.random.default_rng(n + 3)
        x = _exact.family_rows(rng, 0, n, n, width=len(_exact.FAMILIES), blips=(n // 2,)).T
        ends = rng.normal(0, 1, n).astype(np.float32)
        ends[0], ends[-1] = -np.inf, np.inf  # n = 1: the one sample is +inf
        x = np.concatenate([x, np.full((1, n), -7.25, np.float32), ends[None]])
        x.setflags(write=False)
        _ROWS[n] = x
    return _ROWS[n]
