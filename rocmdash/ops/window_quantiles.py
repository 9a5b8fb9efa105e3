"""Window quantile trend: exact percentiles of every trend column. HIP entry + reference.

Kernel: ``csrc/window_quantiles.hip``. The trend keeps ``min / max / mean`` per column and the
heatmap a distribution to the resolution of its bins; this is percentiles over time - "p99 per
10 s for the last hour" - exact, per series and column.

Semantics (stated here once; the geometry is :func:`rocmdash.ops.window_trend.trend_geometry`):

* Columns and slots are the trend's: ``columns = P`` a power of two, ``8 <= P <= 1024``,
  ``P <= W``, ``c = W / P <= 65536`` rows per column, ``P + 1`` slots per series.
* Per (series, slot), over the slot's valid (non-NaN) float32 samples sorted by the kernels'
  key order (``-0.0 < +0.0``), the three percentiles ``pct = (a, b, c)`` by the stats
  kernels' arithmetic (``wanted_positions`` / ``percentile_between`` in
  ``csrc/window_stats_rules.h``), 0-based over ``nv`` valid samples::

      p    = double(float(pct)) / 100 * (nv - 1)
      lo   = floor(p);  hi = min(lo + 1, nv - 1)
      frac = float(p - lo)
      out  = float(frac >= 0.5 ? x1 - (x1 - x0) * (1 - frac) : x0 + (x1 - x0) * frac)

  with ``x0`` / ``x1`` the order statistics at ``lo`` / ``hi`` - selections, never estimates.
  Where the percentile is an order statistic (``frac == 0`` or ``x0 == x1``) and one of the
  two is infinite, it is ``x0`` as it is - the arithmetic would make NaN of ``inf - inf``.
* Output: float32 ``[S, P + 1, 4] = {p_a, p_b, p_c, count}``; ``count`` is the exact number of
  valid samples, bit-identical to the trend's; a slot with no valid sample is
  ``{NaN, NaN, NaN, 0}``.
* Each percentile is finite and in ``[0, 100]``; the default is 50 / 90 / 99.

Reference counterpart: none - the reference shows instant values only.
"""

from __future__ import annotations

import numpy as np

from .window_trend import MAX_STRIDE, MAX_WINDOW, MIN_COLUMNS, check_columns, trend_age_rows, trend_geometry

__all__ = ["DEFAULT_PCT", "Q_COUNT", "check_columns", "check_pct", "trend_age_rows", "trend_geometry",
           "window_quantiles", "window_quantiles_reference"]

DEFAULT_PCT = (50.0, 90.0, 99.0)
Q_COUNT = 3  # the last of a slot's four floats


def check_pct(pct) -> tuple:
    """The three percentiles as floats; ``ValueError`` unless each is finite and in [0, 100]."""
    p = tuple(float(q) for q in pct)
    if len(p) != 3 or not all(0.0 <= q <= 100.0 for q in p):  # NaN fails the comparison
        raise ValueError(f"three percentiles in [0, 100], got {tuple(pct)}")
    return p


def _sort_keys(x: np.ndarray) -> np.ndarray:
    """Order-preserving float32 -> uint32 keys (``fkey`` of csrc/long_window_dev.h)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _key_values(k: np.ndarray) -> np.ndarray:
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _percentiles(v: np.ndarray, pct) -> np.ndarray:
    """The three percentiles of ``v`` (float32, valid, in key order, at least one) - the
    arithmetic of the module docstring in float64, rounded once."""
    last = len(v) - 1
    out = np.empty(3, np.float32)
    for q, pc in enumerate(pct):
        p = float(np.float32(pc)) / 100.0 * float(last)
        lo = min(int(np.floor(p)), last)
        hi = lo + 1 if lo + 1 <= last else last
        f = float(np.float32(p - float(lo)))
        if (f == 0 or v[lo] == v[hi]) and not (np.isfinite(v[lo]) and np.isfinite(v[hi])):
            out[q] = v[lo]
            continue
        x0, x1 = np.float64(v[lo]), np.float64(v[hi])
        with np.errstate(invalid="ignore", over="ignore"):
            out[q] = np.float32(x1 - (x1 - x0) * (1.0 - f) if f >= 0.5 else x0 + (x1 - x0) * f)
    return out


def window_quantiles_reference(rows, head, window, columns, pct=DEFAULT_PCT) -> np.ndarray:
    """Reference, numpy only. ``rows``: ``[n, S]`` float32, oldest first, being rows
    ``head - n .. head - 1``. Returns float32 ``[S, P + 1, 4]``."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2:
        raise ValueError("rows must be [samples, series]")
    pct = check_pct(pct)
    n, S = rows.shape
    _, ranges = trend_geometry(head, n, window, columns)
    out = np.full((S, len(ranges), 4), np.nan, dtype=np.float32)
    out[:, :, Q_COUNT] = 0
    first = int(head) - n
    for j, (b, e) in enumerate(ranges):
        if e <= b:
            continue
        x = rows[b - first : e - first]
        for s in range(S):
            col = x[:, s]
            col = col[~np.isnan(col)]
            out[s, j, Q_COUNT] = len(col)
            if len(col):
                out[s, j, :3] = _percentiles(_key_values(np.sort(_sort_keys(col))), pct)
    return out


def window_quantiles(x, columns, pct=DEFAULT_PCT, head=None, window=None):
    """Run the HIP kernel on a device tensor ``x`` ``[S, n]`` (float32, oldest first, NaN =
    invalid), being rows ``head - n .. head - 1`` (``head`` defaults to n) of a window of
    ``window`` rows (default: the next power of two >= n). The rows are laid into a
    time-major ring of depth ``2 * window`` at their slots, exactly as ``window_trend`` does,
    and ``quantile_ring`` runs on the current stream. Returns float32 ``[S, columns + 1, 4]``
    on the device."""
    import torch

    from ..runtime.native import load

    if not x.is_cuda:
        raise ValueError("window_quantiles runs on a GPU tensor; use window_quantiles_reference on the CPU")
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    pct = check_pct(pct)
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
    load().quantile_ring(ring.data_ptr(), S, S, depth, head, n, int(columns), c, out.data_ptr(),
                         torch.cuda.current_stream(x.device).cuda_stream, *pct)
    return out
