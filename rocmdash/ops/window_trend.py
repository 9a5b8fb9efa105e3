"""Window trend: a window decimated into a chart's worth of columns. HIP entry + reference.

Kernel: ``csrc/window_trend.hip``. Everything else rocmdash reports about a window forgets
*when* things happened; the trend keeps it: per series and column ``{min, max, mean, count}``
of the column's rows.

Semantics (the one statement of them is :func:`trend_geometry`):

* ``columns = P`` is a power of two, ``8 <= P <= 1024`` and ``P <= W``; a column has
  ``c = W / P <= 65536`` rows.
* Columns are anchored to absolute row numbers: row ``r`` (rows ever written, 0-based) is in
  column ``r // c``, so a full column never changes while the window slides over it.
* The window ``[head - n, head)`` touches at most ``P + 1`` aligned columns: the output has
  ``P + 1`` slots, slot ``j`` (0 = oldest, ``P`` = newest) being column
  ``(head - 1) // c - P + j`` cut to the window. Slot ``P`` grows, slot 0 shrinks.
* NaN samples are skipped; ``min`` / ``max`` are exact selections (``-0.0 < +0.0``);
  ``mean`` is an fp64 sum divided in fp64, rounded once; a slot with no valid sample is
  ``{NaN, NaN, NaN, 0}``.

Reference counterpart: none - the reference shows instant values only.
"""

from __future__ import annotations

import numpy as np

MIN_COLUMNS = 8
MAX_COLUMNS = 1024  # csrc/window_trend.h kMaxTrendColumns
MAX_ROWS_PER_COLUMN = 65536  # kMaxTrendRowsPerColumn: one workgroup's stream; counts exact in fp32
MAX_WINDOW = 1 << 26  # the longest window rocmdash keeps (LongWindowSet)
MAX_STRIDE = 64  # kMaxTrendStride: series in one ring
T_MIN, T_MAX, T_MEAN, T_COUNT = 0, 1, 2, 3


def check_columns(columns, window) -> int:
    """Rows per column for ``columns`` over a window of ``window`` rows; ``ValueError``
    unless both are powers of two, ``8 <= columns <= 1024``, ``columns <= window`` and
    ``window / columns <= 65536``."""
    P, W = int(columns), int(window)
    if W < 1 or W & (W - 1):
        raise ValueError(f"window must be a power of two, got {window}")
    if P < MIN_COLUMNS or P > MAX_COLUMNS or P & (P - 1):
        raise ValueError(f"columns must be a power of two in [{MIN_COLUMNS}, {MAX_COLUMNS}], got {columns}")
    if P > W:
        raise ValueError(f"{P} columns for a window of {W} rows")
    if W // P > MAX_ROWS_PER_COLUMN:
        raise ValueError(f"{W // P} rows per column: at most {MAX_ROWS_PER_COLUMN} (more columns for this window)")
    return W // P


def trend_geometry(head, n, window, columns):
    """``(rows_per_col, ranges)`` of the window ``[head - n, head)``: ``ranges`` is int64
    ``[P + 1, 2]``, slot j's rows ``[begin, end)``; ``begin == end`` (both 0) = empty."""
    c = check_columns(columns, window)
    head, n, P = int(head), int(n), int(columns)
    if not 0 <= n <= min(head, int(window)):
        raise ValueError(f"a window of {n} rows at head {head} (window {window})")
    ranges = np.zeros((P + 1, 2), dtype=np.int64)
    if n:
        last = (head - 1) // c
        for j in range(P + 1):
            a = last - P + j
            b, e = max(a * c, head - n), min((a + 1) * c, head)
            if a >= 0 and b < e:
                ranges[j] = b, e
    return c, ranges


def trend_age_rows(head, n, window, columns) -> np.ndarray:
    """float64 ``[P + 1]``: per slot, how many rows before the newest row its last row lies
    (0 for the newest slot; NaN for an empty one) - the chart's x axis, times the period."""
    _, ranges = trend_geometry(head, n, window, columns)
    age = np.full(len(ranges), np.nan)
    full = ranges[:, 1] > ranges[:, 0]
    age[full] = int(head) - ranges[full, 1]
    return age


def window_trend_reference(rows, head, window, columns) -> np.ndarray:
    """Reference, numpy only. ``rows``: ``[n, S]`` float32, oldest first, being rows
    ``head - n .. head - 1``. Returns float32 ``[S, P + 1, 4]``."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2:
        raise ValueError("rows must be [samples, series]")
    n, S = rows.shape
    _, ranges = trend_geometry(head, n, window, columns)
    out = np.full((S, len(ranges), 4), np.nan, dtype=np.float32)
    out[:, :, T_COUNT] = 0
    first = int(head) - n
    for j, (b, e) in enumerate(ranges):
        if e <= b:
            continue
        x = rows[b - first : e - first]
        valid = ~np.isnan(x)
        cnt = valid.sum(axis=0)
        has = cnt > 0
        if not has.any():
            continue
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            # -0.0 < +0.0: numpy's min / max may return either zero, so order by the sign bit too
            lo = np.where(valid, x, np.float32(np.inf)).min(axis=0)
            hi = np.where(valid, x, np.float32(-np.inf)).max(axis=0)
            neg0 = (valid & (x == 0) & np.signbit(x)).any(axis=0)
            pos0 = (valid & (x == 0) & ~np.signbit(x)).any(axis=0)
            lo = np.where((lo == 0) & neg0, np.float32(-0.0), lo)
            hi = np.where((hi == 0) & pos0, np.float32(0.0), np.where(hi == 0, np.float32(-0.0), hi))
            total = np.where(valid, x, np.float32(0)).astype(np.longdouble).sum(axis=0)
            mean = (total / np.maximum(cnt, 1)).astype(np.float64).astype(np.float32)
        out[has, j, T_MIN] = lo.astype(np.float32)[has]
        out[has, j, T_MAX] = hi.astype(np.float32)[has]
        out[has, j, T_MEAN] = mean[has]
        out[:, j, T_COUNT] = cnt
    return out


def window_trend(x, columns, head=None, window=None):
    """Run the HIP kernel on a device tensor ``x`` ``[S, n]`` (float32, oldest first, NaN =
    invalid), being rows ``head - n .. head - 1`` (``head`` defaults to n) of a window of
    ``window`` rows (default: the next power of two >= n). The rows are laid into a
    time-major ring of depth ``2 * window`` at their slots - so an arbitrary ``head``
    exercises the wrap - and ``trend_ring`` runs on the current stream. Returns float32
    ``[S, columns + 1, 4]`` on the device."""
    import torch

    from ..runtime.native import load

    if not x.is_cuda:
        raise ValueError("window_trend runs on a GPU tensor; use window_trend_reference on the CPU")
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    S, n = x.shape
    if not 1 <= S <= MAX_STRIDE:
        raise ValueError(f"1 to {MAX_STRIDE} series in one ring, got {S}")
    if n > MAX_WINDOW:
        raise ValueError(f"window length must be at most {MAX_WINDOW}, got {n}")
    if window is None:
        window = max(MIN_COLUMNS, 1 << max(0, int(n) - 1).bit_length())
    head = n if head is None else int(head)
    c, _ = trend_geometry(head, n, window, columns)  # validates everything
    depth = 2 * int(window)
    ring = torch.full((depth, S), float("nan"), dtype=torch.float32, device=x.device)
    if n:
        slots = (torch.arange(head - n, head, device=x.device, dtype=torch.int64) % depth)
        ring[slots] = x.to(torch.float32).t()
    out = torch.empty((S, int(columns) + 1, 4), dtype=torch.float32, device=x.device)
    load().trend_ring(ring.data_ptr(), S, S, depth, head, n, int(columns), c, out.data_ptr(),
                      torch.cuda.current_stream(x.device).cuda_stream)
    return out
