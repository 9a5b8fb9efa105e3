"""Window joint histogram: two series of one ring binned together. HIP entry + exact integer
reference.

Kernel: ``csrc/window_joint.hip``. Buckets, trend, excursions and heatmap each answer a
question about one series at a time; how two series of the same GPU move together - MFMA
utilization against HBM bandwidth (compute- or memory-bound?), activity against power
(throttled?), power against temperature - none of them can say, because marginals do not
determine a joint distribution, and Prometheus cannot rebuild it: it scrapes once a second
while the rings run at 10 and 100 Hz, so the pairing of the samples of one row is lost before
it arrives. The two values of a pair sit in the same ring row, a few floats apart.

Semantics (stated here once; the headers and everything else point here):

* ``pairs`` is 1 to 8 (``MAX_PAIRS``) ordered pairs ``(a, b)`` of series indices, ``a != b``,
  both series in the same ring. The rows of one ring were sampled at one instant; rows of
  different rings have no common row number and run at different rates, so a pair across rings
  is refused - never silently approximated. A pair may be named twice; it is counted once and
  written to both outputs.
* ``bounds`` are those of ``rocmdash.ops.window_buckets.check_bounds``: ``[S][B]`` float32,
  finite and strictly ascending per series - here ``1 <= B <= 31`` (``MAX_JOINT_BUCKETS``), so
  a pair has ``(B + 1)^2 <= 1024`` cells.
* The bin of a sample ``x`` of series ``s`` is the long buckets' rule, unchanged:
  ``#{k : bounds[s][k] < x}``, compared in fp32: bin ``k`` holds ``bounds[k - 1] < x <=
  bounds[k]``, so ties go down; ``-0.0 == +0.0``; ``-inf`` lands in bin 0 and ``+inf`` in bin
  ``B``.
* A row counts for the pair ``(a, b)`` only when both its samples are not NaN.
* The output is int32 ``[K][B + 1][B + 1]``: ``out[k][i][j]`` is the number of such rows of
  the window with ``bin(x_a) == i`` and ``bin(x_b) == j``. Every cell is written, zeroes
  included; ``n == 0`` (no refresh yet, after ``invalidate()``) is all zeroes.
* Counts are at most 2^26: int32 is exact, and the result depends neither on how the window is
  chunked nor on the order of combination.

Three identities follow: a pair's cells sum to the number of rows where both series are valid;
where neither series has a NaN, the row sums and the column sums are the de-cumulated
``window_buckets`` / ``long_window_buckets`` counts of ``a`` and of ``b``; and ``(b, a)`` is
the transpose of ``(a, b)``.

Reference counterpart: none - the reference shows instant values only.
"""

from __future__ import annotations

import numpy as np

from .window_buckets import MAX_LONG_WINDOW, MAX_RING_STRIDE, check_bounds

MAX_PAIRS = 8  # csrc/window_joint_plan.h kMaxJointPairs
MAX_JOINT_BUCKETS = 31  # csrc/window_joint_plan.h kMaxJointBuckets
DEFAULT_BUCKETS = 16
# kept only where both series exist (GpuAgent.default_joint_pairs); the amd_gpu_ prefix is implied
DEFAULT_PAIRS = (
    ("mfma_utilization", "hbm_read_bandwidth"),
    ("mfma_utilization", "hbm_write_bandwidth"),
    ("gfx_activity", "average_package_power"),
    ("average_package_power", "junction_temperature"),
)
PREFIX = "amd_gpu_"


def check_joint_bounds(bounds, num_series: int | None = None) -> np.ndarray:
    """``check_bounds`` with the joint histogram's ``1 <= B <= 31``."""
    b = check_bounds(bounds, num_series)
    if b.shape[1] > MAX_JOINT_BUCKETS:
        raise ValueError(f"1 to {MAX_JOINT_BUCKETS} bounds per series for a joint histogram, got {b.shape[1]}")
    return b


def check_pairs(pairs, widths) -> list:
    """``pairs`` as a list of ``(a, b)`` ints, checked against a set whose rings have
    ``widths`` series each, in order (one int: one ring): ``ValueError`` unless there are 1 to
    8 pairs, each with ``a != b``, both indices in the set and both in the same ring."""
    widths = [int(widths)] if np.isscalar(widths) else [int(w) for w in widths]
    try:
        out = [(int(a), int(b)) for a, b in pairs]
    except (TypeError, ValueError):
        raise ValueError(f"pairs are [(a, b), ..] series indices, got {pairs!r}") from None
    if not 1 <= len(out) <= MAX_PAIRS:
        raise ValueError(f"1 to {MAX_PAIRS} pairs, got {len(out)}")
    S = sum(widths)
    edges = np.cumsum([0] + widths)
    for a, b in out:
        if a == b:
            raise ValueError(f"a pair needs two different series, got ({a}, {b})")
        if not (0 <= a < S and 0 <= b < S):
            raise ValueError(f"pair ({a}, {b}) names a series beyond the {S} of this set")
        ra, rb = (int(np.searchsorted(edges, v, side="right")) - 1 for v in (a, b))
        if ra != rb:
            raise ValueError(f"pair ({a}, {b}) spans rings {ra} and {rb}: rows of different rings have no common "
                             "row number (they are sampled at different rates), so a cross-ring pair is not counted")
    return out


def parse_joint(spec, series, widths=None) -> tuple:
    """``"default"`` or ``"metricA:metricB,metricC:metricD"``, each with an optional ``/B``
    (default 16), as ``(pairs, B)`` with the pairs as indices into ``series`` (names; the
    ``amd_gpu_`` prefix is optional in the spec). ``default`` keeps those of ``DEFAULT_PAIRS``
    whose two series exist. ``ValueError`` for a malformed spec, an unknown metric, B outside
    1..31 and whatever ``check_pairs`` refuses (``widths``: the rings' widths; default one
    ring)."""
    if not isinstance(spec, str):
        raise ValueError(f"a joint histogram is 'default' or 'metricA:metricB,..' with an optional /B, got {spec!r}")
    series = list(series)
    text, _, btext = spec.strip().partition("/")
    B = DEFAULT_BUCKETS
    if btext or "/" in spec:
        try:
            B = int(btext)
        except ValueError:
            raise ValueError(f"the buckets after '/' must be an integer, got {btext!r}") from None
    if not 1 <= B <= MAX_JOINT_BUCKETS:
        raise ValueError(f"1 to {MAX_JOINT_BUCKETS} buckets for a joint histogram, got {B}")

    def index(name):
        name = name.strip()
        for cand in (name, PREFIX + name):
            if cand in series:
                return series.index(cand)
        raise ValueError(f"unknown metric {name!r} (known: {', '.join(series)})")

    text = text.strip()
    if text == "default":
        names = [(a, b) for a, b in DEFAULT_PAIRS if PREFIX + a in series and PREFIX + b in series]
        if not names:
            raise ValueError("none of the default pairs has both its series here")
    else:
        names = []
        for part in text.split(","):
            ab = part.split(":")
            if len(ab) != 2 or not ab[0].strip() or not ab[1].strip():
                raise ValueError(f"a pair is metricA:metricB, got {part!r}")
            names.append((ab[0], ab[1]))
    pairs = [(index(a), index(b)) for a, b in names]
    return check_pairs(pairs, [len(series)] if widths is None else widths), B


def window_joint_reference(rows, pairs, bounds) -> np.ndarray:
    """Reference, numpy only. ``rows``: ``[n, S]`` float32, the window of one ring (or of a set
    whose pairs were checked by ``check_pairs``); ``pairs``: ``[(a, b), ..]``; ``bounds``:
    ``[S, B]`` or ``[B]``. Returns int32 ``[K, B + 1, B + 1]``."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2:
        raise ValueError("rows must be [samples, series]")
    S = rows.shape[1]
    b = check_joint_bounds(bounds, S)
    pairs = check_pairs(pairs, S)
    B1 = b.shape[1] + 1
    out = np.zeros((len(pairs), B1, B1), dtype=np.int32)
    for k, (i, j) in enumerate(pairs):
        x, y = rows[:, i], rows[:, j]
        both = ~(np.isnan(x) | np.isnan(y))
        # #{k : bounds[k] < x}: the bounds strictly below x (fp32 both; -0.0 == +0.0)
        bx = np.searchsorted(b[i], x[both], side="left")
        by = np.searchsorted(b[j], y[both], side="left")
        out[k] = np.bincount(bx * B1 + by, minlength=B1 * B1).reshape(B1, B1)
    return out


def window_joint(x, pairs, bounds, head=None, window=None, out=None):
    """Run the HIP kernel on a device tensor ``x`` ``[S, n]`` (float32, oldest first, NaN =
    invalid; one ring of S <= 64 series), being rows ``head - n .. head - 1`` (``head``
    defaults to n) of a window of ``window`` rows (default: the next power of two >= n), with
    ``pairs`` and ``bounds`` ``[S, B]`` or ``[B]``. The rows are laid into a time-major ring of
    depth ``2 * window`` at their slots, exactly like ``window_heatmap``, and ``joint_ring``
    runs on the current stream. Returns int32 ``[K, B + 1, B + 1]`` on the device (``out`` when
    given: a contiguous int32 device tensor of that shape, whatever it holds)."""
    import torch

    from ..runtime.native import load

    if not x.is_cuda:
        raise ValueError("window_joint runs on a GPU tensor; use window_joint_reference on the CPU")
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    S, n = x.shape
    if not 1 <= S <= MAX_RING_STRIDE:
        raise ValueError(f"1 to {MAX_RING_STRIDE} series in one ring, got {S}")
    if n > MAX_LONG_WINDOW:
        raise ValueError(f"window length must be at most {MAX_LONG_WINDOW}, got {n}")
    b = check_joint_bounds(bounds.detach().cpu().numpy() if isinstance(bounds, torch.Tensor) else bounds, S)
    pairs = check_pairs(pairs, S)
    if window is None:
        window = max(8, 1 << max(0, int(n) - 1).bit_length())
    window = int(window)
    head = n if head is None else int(head)
    if window < 1 or window & (window - 1) or n > window or n > head:
        raise ValueError(f"{n} rows ending at head {head} are no window of {window} rows (a power of two)")
    depth = 2 * window
    ring = torch.full((depth, S), float("nan"), dtype=torch.float32, device=x.device)
    if n:
        slots = (torch.arange(head - n, head, device=x.device, dtype=torch.int64) % depth)
        ring[slots] = x.to(torch.float32).t()
    bd = torch.from_numpy(np.array(b)).to(x.device)
    B1 = b.shape[1] + 1
    if out is None:
        out = torch.empty((len(pairs), B1, B1), dtype=torch.int32, device=x.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (len(pairs), B1, B1) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"out must be a contiguous int32 [{len(pairs)}, {B1}, {B1}] tensor on {x.device}")
    load().joint_ring(ring.data_ptr(), S, S, depth, head, n, pairs, bd.data_ptr(), b.shape[1], out.data_ptr(),
                      torch.cuda.current_stream(x.device).cuda_stream)
    return out
