"""Window distributions as cumulative ``le`` buckets: HIP entry + exact integer reference.

Kernel: ``csrc/window_buckets.hip`` (one wave64 per series: lane ``b`` counts the window
samples <= bound ``b`` with one ``upper_bound`` in the series' sorted window, lane ``B``
writes the valid count); for windows of more than 32768 samples, which keep no sorted
state, ``csrc/long_window_buckets.hip`` (one stream of the time-major ring into per-series
histograms, float64 counts). Per series the result is ``B + 1`` counts: the valid (non-NaN)
samples ``x <= bounds[b]`` (fp32 compare: ties count, ``-0.0 == +0.0``, a ``-inf`` sample
is in every bucket, a ``+inf`` sample only in the last), then the valid count, Prometheus'
``+Inf`` bucket. Unlike a percentile, buckets add up: across GPUs, nodes and scrapes,

    histogram_quantile(0.99, sum by (le) (rocmdash_window_bucket{metric="..."}))

and they answer "what share of the last W samples was above 95 C?" (:func:`share_above`).

Reference counterpart: none - the reference shows instant values only (``app.py:216-221``).
"""

from __future__ import annotations

import numpy as np

from ..models.schema import METRIC_SPECS
from .window_stats import MAX_WINDOW

MAX_BUCKETS = 63  # finite bounds per series (csrc/window_buckets.h kMaxBuckets)
MAX_LONG_WINDOW = 1 << 26  # the longest window rocmdash keeps (LongWindowSet)
MAX_RING_STRIDE = 64  # floats per ring row (csrc/long_window_buckets.h kMaxBucketStride)
POWER = "amd_gpu_average_package_power"
VRAM = ("amd_gpu_used_vram", "amd_gpu_total_vram")
DEFAULT_TOTAL_VRAM_MB = 288 * 1024  # an MI355X's HBM, when the GPU's own figure is unknown


def check_bounds(bounds, num_series: int | None = None) -> np.ndarray:
    """``bounds`` ([S, B] or [B]) as float32 [S, B]; ``ValueError`` unless every row is
    finite and strictly ascending (in fp32) with 1 <= B <= 63."""
    b = np.asarray(bounds, dtype=np.float32)
    if b.ndim == 1 and num_series is not None:
        b = np.broadcast_to(b, (num_series, b.shape[0]))
    if b.ndim != 2:
        raise ValueError("bounds must be [series, buckets] or [buckets]")
    if num_series is not None and b.shape[0] != num_series:
        raise ValueError(f"bounds are for {b.shape[0]} series, not {num_series}")
    if not 1 <= b.shape[1] <= MAX_BUCKETS:
        raise ValueError(f"1 to {MAX_BUCKETS} bounds per series, got {b.shape[1]}")
    if not np.all(np.isfinite(b)):
        raise ValueError("bounds must be finite (the +Inf bucket is always added)")
    if b.shape[1] > 1 and not np.all(b[:, 1:] > b[:, :-1]):
        raise ValueError("bounds must be strictly ascending per series")
    return np.ascontiguousarray(b)


def window_buckets_reference(x, bounds) -> np.ndarray:
    """Exact reference. ``x``: [S, n] samples, oldest first, NaN = invalid; ``bounds``:
    [S, B] or [B]. Returns int64 [S, B + 1]: per series the valid fp32 samples <= each fp32
    bound, then the valid count."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    S = x.shape[0]
    b = check_bounds(bounds, S)
    out = np.zeros((S, b.shape[1] + 1), dtype=np.int64)
    for s in range(S):
        v = np.sort(x[s][~np.isnan(x[s])])
        out[s, :-1] = np.searchsorted(v, b[s], side="right")
        out[s, -1] = v.size
    return out


def bucket_ring_reference(rows, head: int, n: int, bounds) -> np.ndarray:
    """Exact reference of ``bucket_ring``. ``rows``: host ``[depth, stride]``, a time-major
    ring with row r at slot ``r & (depth - 1)`` (depth a power of two), whose window is rows
    ``[head - n, head)``; ``bounds``: ``[cols, B]`` for the ring's first ``cols`` columns
    (or ``[B]``: every column). Returns int64 ``[cols, B + 1]``."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2:
        raise ValueError("rows must be [depth, stride]")
    depth, stride = rows.shape
    head, n = int(head), int(n)
    if depth < 1 or depth & (depth - 1):
        raise ValueError(f"the ring depth must be a power of two, got {depth}")
    if not 0 <= n <= min(depth, head):
        raise ValueError(f"a window of {n} rows does not fit a ring of {depth} rows at head {head}")
    b = np.asarray(bounds, dtype=np.float32)
    cols = stride if b.ndim == 1 else b.shape[0]
    if not 1 <= cols <= stride:
        raise ValueError(f"bounds are for {cols} series, the ring has {stride} columns")
    slots = (np.arange(head - n, head, dtype=np.int64) & (depth - 1)) if n else np.zeros(0, np.int64)
    return window_buckets_reference(rows[slots, :cols].T.reshape(cols, n), b)


def long_window_buckets(x, bounds):
    """``window_buckets`` for 32768 < n <= 2^26 samples per series (S <= 64), which no sorted
    window holds: ``x`` [S, n] (device, float32, oldest first, NaN = invalid) is laid out
    time-major as the first n rows of a ring of the next power-of-two depth and streamed
    once by ``bucket_ring`` (csrc/long_window_buckets.hip) on the current stream. Returns
    float64 [S, B + 1] on the device: a count may pass 2^24, where float32 stops being
    exact. Shorter windows are accepted too (the same counts as ``window_buckets``)."""
    import torch

    from ..runtime.native import load

    if not x.is_cuda:
        raise ValueError("long_window_buckets runs on a GPU tensor; use window_buckets_reference on the CPU")
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    S, n = x.shape
    if n < 1 or n > MAX_LONG_WINDOW:
        raise ValueError(f"window length must be in [1, {MAX_LONG_WINDOW}], got {n}")
    if S > MAX_RING_STRIDE:
        raise ValueError(f"at most {MAX_RING_STRIDE} series per call, got {S}")
    b = np.array(check_bounds(bounds.detach().cpu().numpy() if isinstance(bounds, torch.Tensor) else bounds, S))
    depth = 1 << (n - 1).bit_length()
    ring = torch.full((depth, S), float("nan"), dtype=torch.float32, device=x.device)
    ring[:n] = x.to(torch.float32).T
    bd = torch.from_numpy(b).to(x.device)
    out = torch.empty((S, b.shape[1] + 1), dtype=torch.float64, device=x.device)
    load().bucket_ring(ring.data_ptr(), S, S, depth, n, n, bd.data_ptr(), b.shape[1], out.data_ptr(),
                       torch.cuda.current_stream(x.device).cuda_stream)
    return out


def window_buckets(x, bounds):
    """Run the HIP kernel on a device tensor ``x`` [S, n] (float32, oldest first, NaN =
    invalid) with ``bounds`` [S, B] or [B]; returns float32 [S, B + 1] on the device
    (exact counts: n <= 32768 < 2^24; longer windows: ``long_window_buckets``). The window
    is sorted with torch into one export block ``[1, S, 1 + n]`` (count, ascending samples,
    +inf) and counted by ``bucket_blocks`` on the current stream."""
    import torch

    from ..runtime.native import load

    if not x.is_cuda:
        raise ValueError("window_buckets runs on a GPU tensor; use window_buckets_reference on the CPU")
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    S, n = x.shape
    if n < 1 or n > MAX_WINDOW:
        raise ValueError(f"window length must be in [1, {MAX_WINDOW}], got {n}")
    b = check_bounds(bounds.detach().cpu().numpy() if isinstance(bounds, torch.Tensor) else bounds, S)
    B = b.shape[1]
    nat = load()
    xs = x.to(torch.float32)
    nan = torch.isnan(xs)
    block = torch.empty((1, S, 1 + n), dtype=torch.float32, device=x.device)
    block[0, :, 0] = (n - nan.sum(dim=1)).to(torch.float32)
    # NaNs to +inf: they sort last and lie past the count, like an export block's padding
    block[0, :, 1:] = torch.sort(torch.where(nan, torch.full_like(xs, float("inf")), xs), dim=1).values
    bd = torch.from_numpy(b).to(x.device)
    out = torch.empty((S, B + 1), dtype=torch.float32, device=x.device)
    nat.bucket_blocks(block.data_ptr(), 1, S, n, bd.data_ptr(), B, 0, out.data_ptr(),
                      torch.cuda.current_stream(x.device).cuda_stream)
    return out


def default_bounds(series, power_limit_w=None, total_vram_mb=None, buckets: int = 16, card_model=None) -> np.ndarray:
    """[S, B] float32: per series ``buckets`` evenly spaced upper bounds ending at the
    series' axis maximum - ``METRIC_SPECS[...].axis_max``; for power the GPU's cap (unknown:
    the power axis the page picks for ``card_model``, ``viz.panels.power_axis_max``); for
    used and total VRAM the GPU's total VRAM (unknown: an MI355X's)."""
    from ..viz.panels import power_axis_max

    if not 1 <= int(buckets) <= MAX_BUCKETS:
        raise ValueError(f"1 to {MAX_BUCKETS} buckets, got {buckets}")
    B = int(buckets)
    out = np.empty((len(series), B), dtype=np.float32)
    for i, name in enumerate(series):
        if name == POWER:
            top = power_axis_max(card_model, power_limit_w)
        elif name in VRAM:
            ok = total_vram_mb is not None and total_vram_mb == total_vram_mb and total_vram_mb > 0
            top = total_vram_mb if ok else DEFAULT_TOTAL_VRAM_MB
        else:
            spec = METRIC_SPECS.get(name)
            top = spec.axis_max if spec is not None and spec.axis_max else 100.0
        out[i] = np.arange(1, B + 1, dtype=np.float64) * float(top) / B  # the last one is the axis itself
    return check_bounds(out)


def share_above(counts, bounds, threshold: float) -> float:
    """Fraction of the valid samples above the largest bound <= ``threshold`` (``counts``
    [B + 1], ``bounds`` [B] of one series). NaN with no valid sample or no such bound."""
    counts = np.asarray(counts, dtype=np.float64)
    bounds = np.asarray(bounds, dtype=np.float64)
    k = int(np.searchsorted(bounds, threshold, side="right")) - 1
    total = counts[-1]
    if k < 0 or not total > 0:
        return float("nan")
    return float((total - counts[k]) / total)
