"""Window period trend: the autocorrelation's exact integer lag sums per trend column of every
series, and each column's period. HIP entry + exact integer reference.

Kernel: ``csrc/window_periods.hip``. ``window_autocorr`` returns one period per series over the
newest ``span`` rows; "the moment it changes tells when the job slowed down", and one number
cannot show a moment: a period that went from 41 to 55 samples twenty minutes ago looks like 55
now, an hour that alternates between two step times looks like a weak period. Levels have stats
and the trend, percentiles the quantile trend; this is the trend of the rhythm.

Semantics (stated here once; the headers and everything else point here):

* **Options.** ``span`` is a power of two, ``2^9 <= span <= 2^20`` (``MIN_SPAN``, ``MAX_SPAN``),
  default ``min(W, 65536)``, and ``span <= W``. ``P`` is a power of two in ``8 .. 64``. A column
  has ``c = span / P`` rows, ``64 <= c <= 65536``. ``1 <= L <= min(1024, c / 2)``: every lag of
  a full, NaN-free column then has ``2 n_k >= n_0``, so its ``acf`` is defined. ``P (L + 1) <=
  16384`` caps the output at 532 KB of int64 per series. The default ``L`` is 255: at the
  default span and ``P = 64``, ``c = 1024`` and the 256 lags fill exactly one lag block of the
  kernel. :func:`check_periods` raises ``ValueError`` naming the violated rule;
  :func:`parse_periods` takes ``"P"``, ``"P/L"`` or ``"P/L/SPAN"``.
* **Slots.** With ``n' = min(n, span)`` the slots are ``trend_geometry(head, n', span, P)`` of
  ``rocmdash.ops.window_trend``: the trend's ``P + 1`` slots for a window of ``span`` rows,
  columns anchored to absolute row numbers. When ``span == W`` they are the trend's own slots.
  :func:`periods_age_rows` is ``trend_age_rows`` with the same arguments.
* **Sums.** Slot ``j`` with rows ``[b, e)`` holds the four sums ``{n, Sx, Sy, Sxy}`` of
  ``rocmdash.ops.window_autocorr`` of those rows alone: a pair ``(t, t + k)`` counts only when
  ``b <= t`` and ``t + k < e``. Quantisation and ``scale`` are the autocorrelation's
  (``quantise``, ``check_scale``, ``default_scale`` are imported from there). The output is
  int64 ``[S][P + 1][L + 1][4]``; every word is written; an empty slot and every lag ``k >= e -
  b`` are all zero. Per non-empty slot the reference is
  ``window_autocorr_reference(rows[b:e], scale, L, span=MAX_SPAN)``.
* **Period per slot** (host only). :func:`slot_periods` applies the autocorrelation's
  ``correlogram`` and ``pick_period``, unchanged, to every ``[L + 1, 4]`` block: ``(period,
  strength, rows_valid)``, each ``[S, P + 1]``; no period is NaN for period and strength;
  ``rows_valid`` is ``n_0``. The period is in samples.

Out of scope: memoising full columns between calls (the anchoring makes it possible), a
period-change gauge, periods in seconds.

Reference counterpart: none - the reference shows instant values only.
"""

from __future__ import annotations

import numpy as np

from .window_autocorr import (MAX_LAGS, MAX_SPAN, check_scale, correlogram, default_scale, pick_period,  # noqa: F401
                              quantise, window_autocorr_reference)
from .window_buckets import MAX_LONG_WINDOW, MAX_RING_STRIDE
from .window_trend import trend_age_rows, trend_geometry

MIN_SPAN = 1 << 9  # csrc/window_periods.h kMinPeriodsSpan
DEFAULT_SPAN = 1 << 16
MIN_COLUMNS = 8  # kMinPeriodsColumns
MAX_COLUMNS = 64  # kMaxPeriodsColumns
MIN_ROWS_PER_COLUMN = 64  # kMinPeriodsRowsPerColumn
MAX_ROWS_PER_COLUMN = 65536  # kMaxPeriodsRowsPerColumn
MAX_WORDS = 16384  # kMaxPeriodsWords: P x (L + 1)
DEFAULT_LAGS = 255


def check_periods(P, L=None, span=None, window=None) -> tuple:
    """``(P, L, span)`` as ints (``L`` None: 255; ``span`` None: ``min(window, 65536)``, 65536
    without a window): ``ValueError``, naming the rule, unless the options above hold."""
    try:
        vals = []
        for x, default in ((P, None), (L, DEFAULT_LAGS), (span, None)):
            x = default if x is None else x
            if x is not None and (isinstance(x, bool) or int(x) != x):
                raise ValueError
            vals.append(None if x is None else int(x))
        P, L, span = vals
        if P is None:
            raise ValueError
        window = None if window is None else int(window)
    except (TypeError, ValueError):
        raise ValueError(f"columns, lags and span are integers, got {P!r}, {L!r} and {span!r}") from None
    if span is None:
        span = DEFAULT_SPAN if window is None else min(window, DEFAULT_SPAN)
    if not MIN_SPAN <= span <= MAX_SPAN or span & (span - 1):
        raise ValueError(f"the span is a power of two in [{MIN_SPAN}, {MAX_SPAN}], got {span}")
    if window is not None and span > window:
        raise ValueError(f"the span is at most the window: span {span}, window {window}")
    if not MIN_COLUMNS <= P <= MAX_COLUMNS or P & (P - 1):
        raise ValueError(f"columns are a power of two in [{MIN_COLUMNS}, {MAX_COLUMNS}], got {P}")
    c = span // P
    if not MIN_ROWS_PER_COLUMN <= c <= MAX_ROWS_PER_COLUMN:
        raise ValueError(f"{c} rows per column (span {span} / {P} columns): {MIN_ROWS_PER_COLUMN} to {MAX_ROWS_PER_COLUMN}")
    if not 1 <= L <= MAX_LAGS:
        raise ValueError(f"1 to {MAX_LAGS} lags, got {L}")
    if 2 * L > c:
        raise ValueError(f"{L} lags need columns of at least {2 * L} rows, a column has {c}")
    if P * (L + 1) > MAX_WORDS:
        raise ValueError(f"columns x (lags + 1) is at most {MAX_WORDS}, got {P} x {L + 1} = {P * (L + 1)}")
    return P, L, span


def parse_periods(spec, window=None) -> tuple:
    """``"P"``, ``"P/L"`` or ``"P/L/SPAN"`` (or a tuple of one to three ints, or an int) as
    ``(P, L, span)``, checked by ``check_periods``."""
    if isinstance(spec, (tuple, list)) and 1 <= len(spec) <= 3:
        return check_periods(*spec, *([None] * (3 - len(spec))), window)
    if isinstance(spec, (int, np.integer)) and not isinstance(spec, bool):
        return check_periods(spec, None, None, window)
    if not isinstance(spec, str):
        raise ValueError(f"a window period trend is 'P', 'P/L' or 'P/L/SPAN', got {spec!r}")
    parts = spec.strip().split("/")
    try:
        if not 1 <= len(parts) <= 3:
            raise ValueError
        vals = [int(p) for p in parts]
    except ValueError:
        raise ValueError(f"a window period trend is 'P', 'P/L' or 'P/L/SPAN' with integers, got {spec!r}") from None
    return check_periods(*vals, *([None] * (3 - len(vals))), window)


def periods_geometry(head, n, P, span):
    """``(rows_per_col, ranges)``: ``trend_geometry(head, min(n, span), span, P)``."""
    return trend_geometry(head, min(int(n), int(span)), span, P)


def periods_age_rows(head, n, P, span) -> np.ndarray:
    """float64 ``[P + 1]``: ``trend_age_rows(head, min(n, span), span, P)`` - the chart's x axis."""
    return trend_age_rows(head, min(int(n), int(span)), span, P)


def window_periods_reference(rows, scale, head, window, P, L, span=None) -> np.ndarray:
    """Reference, numpy only. ``rows``: ``[n, S]`` float32, oldest first, being rows ``head - n
    .. head - 1`` of a window of ``window`` rows. Returns int64 ``[S, P + 1, L + 1, 4]``: per
    non-empty slot the autocorrelation's reference over the slot's rows."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2:
        raise ValueError("rows must be [samples, series]")
    P, L, span = check_periods(P, L, span, window)
    n, S = rows.shape
    scale = check_scale(scale, S)
    first = int(head) - n
    _, ranges = periods_geometry(head, n, P, span)
    out = np.zeros((S, P + 1, L + 1, 4), dtype=np.int64)
    for j, (b, e) in enumerate(ranges):
        if e > b:
            out[:, j] = window_autocorr_reference(rows[b - first : e - first], scale, L, span=MAX_SPAN)
    return out


def slot_periods(sums) -> tuple:
    """``(period, strength, rows_valid)`` of sums ``[S, P + 1, L + 1, 4]``: float64, float64 and
    int64 ``[S, P + 1]``; ``correlogram`` and ``pick_period`` per block, NaN where there is no
    period; ``rows_valid`` is ``n_0``."""
    sums = np.asarray(sums)
    if sums.ndim != 4 or sums.shape[3] != 4:
        raise ValueError("sums must be [series, columns + 1, lags + 1, 4]")
    S, slots = sums.shape[:2]
    period = np.full((S, slots), np.nan)
    strength = np.full((S, slots), np.nan)
    for s in range(S):
        for j in range(slots):
            k, a = pick_period(correlogram(sums[s, j]))
            if k is not None:
                period[s, j], strength[s, j] = k, a
    return period, strength, sums[:, :, 0, 0].astype(np.int64)


def window_periods(x, scale, P, L=DEFAULT_LAGS, span=None, head=None, window=None, out=None, split=0):
    """Run the HIP kernel on a device tensor ``x`` ``[S, n]`` (float32, oldest first, NaN =
    invalid; one ring of S <= 64 series), being rows ``head - n .. head - 1`` (``head``
    defaults to n) of a window of ``window`` rows (default: the next power of two >= n, at
    least 512). The rows are laid into a time-major ring of depth ``2 * window`` at their slots,
    exactly like ``window_autocorr``, and ``periods_ring`` runs on the current stream. ``split``:
    0 lets the kernel's plan decide, 1 forces a workgroup per slot, a larger power of two that
    many workgroups per slot. Returns int64 ``[S, P + 1, L + 1, 4]`` on the device (``out`` when
    given: a contiguous int64 device tensor of that shape, whatever it holds)."""
    import torch

    from ..runtime.native import load

    if not x.is_cuda:
        raise ValueError("window_periods runs on a GPU tensor; use window_periods_reference on the CPU")
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    S, n = x.shape
    if not 1 <= S <= MAX_RING_STRIDE:
        raise ValueError(f"1 to {MAX_RING_STRIDE} series in one ring, got {S}")
    if n > MAX_LONG_WINDOW:
        raise ValueError(f"window length must be at most {MAX_LONG_WINDOW}, got {n}")
    if window is None:
        window = max(MIN_SPAN, 1 << max(0, int(n) - 1).bit_length())
    window = int(window)
    P, L, span = check_periods(P, L, span, window)
    sc = check_scale(scale.detach().cpu().numpy() if isinstance(scale, torch.Tensor) else scale, S)
    head = n if head is None else int(head)
    if window < 1 or window & (window - 1) or n > window or n > head:
        raise ValueError(f"{n} rows ending at head {head} are no window of {window} rows (a power of two)")
    depth = 2 * window
    ring = torch.full((depth, S), float("nan"), dtype=torch.float32, device=x.device)
    if n:
        slots = (torch.arange(head - n, head, device=x.device, dtype=torch.int64) % depth)
        ring[slots] = x.to(torch.float32).t()
    sd = torch.from_numpy(sc).to(x.device)
    shape = (S, P + 1, L + 1, 4)
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=x.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"out must be a contiguous int64 {list(shape)} tensor on {x.device}")
    load().periods_ring(ring.data_ptr(), S, S, depth, head, n, span, P, sd.data_ptr(), L, out.data_ptr(), int(split),
                        torch.cuda.current_stream(x.device).cuda_stream)
    return out
