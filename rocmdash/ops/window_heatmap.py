"""Window heatmap: the distribution of a window over time. HIP entry + exact integer reference.

Kernel: ``csrc/window_heatmap.hip``. The buckets (``rocmdash.ops.window_buckets``) say how
much of a window lay at each level and forget when; the trend (``rocmdash.ops.window_trend``)
keeps when and forgets everything but min / max / mean. The heatmap keeps both: per series
and column of the window, the count of samples in each bucket - time on x, level on y, count
as colour; the view that tells "300 W in compute and 120 W in communication" from "noisy
around 210 W".

Semantics (stated here once; the header and everything else point here):

* ``columns = P`` and the slots are exactly those of
  ``rocmdash.ops.window_trend.trend_geometry(head, n, window, P)``: ``P`` a power of two in
  ``[8, 1024]``, ``P <= W``, ``W / P <= 65536`` rows per column, ``P + 1`` slots with slot 0
  the oldest, columns anchored to absolute row numbers.
* ``bounds`` are those of ``rocmdash.ops.window_buckets.check_bounds``: ``[S][B]`` float32,
  finite and strictly ascending per series, ``1 <= B <= 63``.
* A valid sample ``x`` of series ``s`` falls in bin ``#{b : bounds[s][b] < x}``, compared in
  fp32 (the rule of ``csrc/long_window_buckets.h``): bin ``k`` holds ``bounds[k - 1] < x <=
  bounds[k]``, so ties go down; ``-0.0 == +0.0``; ``-inf`` lands in bin 0 and ``+inf`` in
  bin ``B``; NaN is skipped.
* The output is int32 ``[S][P + 1][B + 1]`` of per-bin counts - NOT cumulative: a heatmap
  draws bins. Every count is at most 65536; an empty slot is all zeroes, and so is
  ``n == 0``.

Two identities follow: per (series, slot) the bins sum to the trend's ``count`` of that
slot; per series the slots summed and then cumulated over the bins are the
``window_buckets`` / ``long_window_buckets`` counts of the same window.

Reference counterpart: none - the reference shows instant values only.
"""

from __future__ import annotations

import numpy as np

from .window_buckets import MAX_BUCKETS, check_bounds
from .window_trend import MAX_COLUMNS, MAX_STRIDE, MAX_WINDOW, MIN_COLUMNS, trend_geometry

RINGS_PER_LAUNCH = 8  # csrc/window_heatmap.h kHeatmapRingsPerLaunch
MAX_COUNT = 65536  # rows of one column (csrc/window_trend.h kMaxTrendRowsPerColumn)
DEFAULT_COLUMNS = 64
DEFAULT_BUCKETS = 16


def parse_heatmap(spec) -> tuple:
    """``"64x16"`` (or a ``(P, B)`` pair) as ``(P, B)``: ``ValueError`` unless P is a power of
    two in [8, 1024] and 1 <= B <= 63. Whether P fits a window is ``check_columns``' to say."""
    if isinstance(spec, str):
        parts = spec.strip().lower().split("x")
        if len(parts) != 2:
            raise ValueError(f"a heatmap is COLUMNSxBUCKETS, e.g. 64x16, got {spec!r}")
        try:
            P, B = int(parts[0]), int(parts[1])
        except ValueError:
            raise ValueError(f"a heatmap is COLUMNSxBUCKETS, e.g. 64x16, got {spec!r}") from None
    else:
        try:
            P, B = (int(v) for v in spec)
        except (TypeError, ValueError):
            raise ValueError(f"a heatmap is (columns, buckets), got {spec!r}") from None
    if P < MIN_COLUMNS or P > MAX_COLUMNS or P & (P - 1):
        raise ValueError(f"columns must be a power of two in [{MIN_COLUMNS}, {MAX_COLUMNS}], got {P}")
    if not 1 <= B <= MAX_BUCKETS:
        raise ValueError(f"1 to {MAX_BUCKETS} buckets, got {B}")
    return P, B


def window_heatmap_reference(rows, head, window, columns, bounds) -> np.ndarray:
    """Reference, numpy only. ``rows``: ``[n, S]`` float32, oldest first, being rows
    ``head - n .. head - 1``; ``bounds``: ``[S, B]`` or ``[B]``. Returns int32
    ``[S, P + 1, B + 1]``."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2:
        raise ValueError("rows must be [samples, series]")
    n, S = rows.shape
    b = check_bounds(bounds, S)
    _, ranges = trend_geometry(head, n, window, columns)
    B = b.shape[1]
    out = np.zeros((S, len(ranges), B + 1), dtype=np.int32)
    first = int(head) - n
    for j, (lo, hi) in enumerate(ranges):
        if hi <= lo:
            continue
        x = rows[lo - first : hi - first]
        for s in range(S):
            v = x[:, s]
            v = v[~np.isnan(v)]
            # #{b : bounds[b] < x}: the bounds strictly below x (fp32 both; -0.0 == +0.0)
            out[s, j] = np.bincount(np.searchsorted(b[s], v, side="left"), minlength=B + 1)
    return out


def window_heatmap(x, columns, bounds, head=None, window=None):
    """Run the HIP kernel on a device tensor ``x`` ``[S, n]`` (float32, oldest first, NaN =
    invalid), being rows ``head - n .. head - 1`` (``head`` defaults to n) of a window of
    ``window`` rows (default: the next power of two >= n), with ``bounds`` ``[S, B]`` or
    ``[B]``. The rows are laid into a time-major ring of depth ``2 * window`` at their slots,
    exactly like ``window_trend``, and ``heatmap_ring`` runs on the current stream. Returns
    int32 ``[S, columns + 1, B + 1]`` on the device."""
    import torch

    from ..runtime.native import load

    if not x.is_cuda:
        raise ValueError("window_heatmap runs on a GPU tensor; use window_heatmap_reference on the CPU")
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    S, n = x.shape
    if not 1 <= S <= MAX_STRIDE:
        raise ValueError(f"1 to {MAX_STRIDE} series in one ring, got {S}")
    if n > MAX_WINDOW:
        raise ValueError(f"window length must be at most {MAX_WINDOW}, got {n}")
    b = check_bounds(bounds.detach().cpu().numpy() if isinstance(bounds, torch.Tensor) else bounds, S)
    if window is None:
        window = max(MIN_COLUMNS, 1 << max(0, int(n) - 1).bit_length())
    head = n if head is None else int(head)
    c, _ = trend_geometry(head, n, window, columns)  # validates everything
    depth = 2 * int(window)
    ring = torch.full((depth, S), float("nan"), dtype=torch.float32, device=x.device)
    if n:
        slots = (torch.arange(head - n, head, device=x.device, dtype=torch.int64) % depth)
        ring[slots] = x.to(torch.float32).t()
    bd = torch.from_numpy(np.array(b)).to(x.device)
    out = torch.empty((S, int(columns) + 1, b.shape[1] + 1), dtype=torch.int32, device=x.device)
    load().heatmap_ring(ring.data_ptr(), S, S, depth, head, n, int(columns), c, bd.data_ptr(), b.shape[1],
                        out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream)
    return out
