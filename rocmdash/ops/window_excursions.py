"""Window excursions: the episodes a window spent above a threshold. HIP entry + reference.

Kernel: ``csrc/window_excursions.hip`` (the combine: ``csrc/window_excursions_monoid.h``).
Statistics, buckets and trend say how much of a window lay above a level; this says how
*often*, for how long at worst, and whether it is above right now - the only reduction here
in which the order of the samples is the result.

Semantics (this is the one statement of them):

* ``1 <= K <= 4`` thresholds per series, finite and strictly increasing within a series
  (:func:`check_thresholds`).
* The reduction runs over the window rows ``[head - n, head)`` of a series, oldest first.
* A NaN sample is skipped: it neither ends nor extends an episode. All lengths are counted
  in valid samples.
* A valid sample is *above* when ``x > t``, strictly (fp32 compare): ``+inf`` is above, a
  sample equal to the threshold is not.
* An *episode* is a maximal run of above samples in the sequence of valid samples. A run
  cut by the oldest edge of the window counts as an episode.
* Per (series, threshold) one record of eight int32, ``[S][K][8]``:

  ===  ============  ==========================================================================
  0    ``above``     valid samples above the threshold
  1    ``valid``     valid samples
  2    ``episodes``  number of episodes
  3    ``longest``   length of the longest episode (0 if none)
  4    ``current``   length of the episode that contains the newest valid sample (0 if that
                     sample is not above)
  5    ``since``     valid samples after the end of the last episode (0 while ``current > 0``;
                     ``valid`` when there is no episode)
  6    ``leading``   length of the episode that contains the oldest valid sample (0 if that
                     sample is not above); when ``> 0`` it may have begun before the window
  7    ``rows``      ``n``, invalid rows included
  ===  ============  ==========================================================================

* ``n == 0`` gives all zeroes, an all-NaN series zeroes with ``rows = n``. Every value is at
  most 2^26: int32 is exact.

Partials of adjacent time ranges combine in an associative, non-commutative monoid over
``(len, above, pre, suf, longest, episodes, tail_below)`` (:func:`excursion_combine`): the
kernel cuts the window into chunks, waves and lanes and folds them back in time order, so
any cut gives the same integers.

Reference counterpart: none - the reference shows instant values only.
"""

from __future__ import annotations

import numpy as np

MAX_THRESHOLDS = 4  # csrc/window_excursions.h kMaxExcursionThresholds
MAX_CHUNKS = 1024  # kMaxExcursionChunks: chunks of one ring's window
MAX_WINDOW = 1 << 26  # the longest window rocmdash keeps (LongWindowSet)
MAX_STRIDE = 64  # kMaxExcursionStride: series in one ring
FIELDS = ("above", "valid", "episodes", "longest", "current", "since", "leading", "rows")
E_ABOVE, E_VALID, E_EPISODES, E_LONGEST, E_CURRENT, E_SINCE, E_LEADING, E_ROWS = range(8)
# a partial: the monoid's words, in the order of csrc/window_excursions_monoid.h
P_LEN, P_ABOVE, P_PRE, P_SUF, P_LONGEST, P_EPISODES, P_TAIL_BELOW = range(7)
IDENTITY = (0, 0, 0, 0, 0, 0, 0)


def check_thresholds(thresholds, num_series: int | None = None) -> np.ndarray:
    """``thresholds`` ([S, K] or [K]) as float32 [S, K]; ``ValueError`` unless every row is
    finite and strictly increasing (in fp32) with 1 <= K <= 4."""
    t = np.asarray(thresholds, dtype=np.float32)
    if t.ndim == 1 and num_series is not None:
        t = np.broadcast_to(t, (num_series, t.shape[0]))
    if t.ndim != 2:
        raise ValueError("thresholds must be [series, thresholds] or [thresholds]")
    if num_series is not None and t.shape[0] != num_series:
        raise ValueError(f"thresholds are for {t.shape[0]} series, not {num_series}")
    if not 1 <= t.shape[1] <= MAX_THRESHOLDS:
        raise ValueError(f"1 to {MAX_THRESHOLDS} thresholds per series, got {t.shape[1]}")
    if not np.all(np.isfinite(t)):
        raise ValueError("thresholds must be finite")
    if t.shape[1] > 1 and not np.all(t[:, 1:] > t[:, :-1]):
        raise ValueError("thresholds must be strictly increasing per series")
    return np.ascontiguousarray(t)


def parse_fractions(text) -> tuple[float, ...]:
    """``"0.5,0.9"`` (or a sequence of numbers) as a tuple of 1 to 4 strictly increasing
    fractions in (0, 1]; ``ValueError`` otherwise. The exporter's ``--window-excursions``."""
    parts = [p.strip() for p in text.split(",")] if isinstance(text, str) else list(text)
    try:
        fr = tuple(float(p) for p in parts)
    except (TypeError, ValueError):
        raise ValueError(f"fractions must be numbers, got {text!r}") from None
    if not 1 <= len(fr) <= MAX_THRESHOLDS:
        raise ValueError(f"1 to {MAX_THRESHOLDS} fractions, got {len(fr)}")
    if not all(0.0 < f <= 1.0 for f in fr):  # NaN fails too
        raise ValueError(f"fractions must lie in (0, 1], got {text!r}")
    if any(b <= a for a, b in zip(fr, fr[1:])):
        raise ValueError(f"fractions must be strictly increasing, got {text!r}")
    return fr


def excursion_combine(a, b):
    """Partial of time range ``a`` followed by ``b``: tuples ``(len, above, pre, suf,
    longest, episodes, tail_below)``. Associative, not commutative; :data:`IDENTITY` (the
    empty range) is its identity."""
    alen, aabove, apre, asuf, alongest, aep, atail = (int(v) for v in a)
    blen, babove, bpre, bsuf, blongest, bep, btail = (int(v) for v in b)
    return (
        alen + blen,
        aabove + babove,
        alen + bpre if apre == alen else apre,
        blen + asuf if bsuf == blen else bsuf,
        max(alongest, blongest, asuf + bpre),
        aep + bep - int(asuf > 0 and bpre > 0),
        blen + atail if btail == blen else btail,
    )


def partial_of_record(rec):
    """The monoid partial a record (8 integers) was written from."""
    r = [int(v) for v in rec]
    return (r[E_VALID], r[E_ABOVE], r[E_LEADING], r[E_CURRENT], r[E_LONGEST], r[E_EPISODES], r[E_SINCE])


def record_of_partial(p, rows: int) -> np.ndarray:
    """The record of a whole window of ``rows`` rows whose partial is ``p``."""
    out = np.zeros(8, dtype=np.int32)
    out[[E_VALID, E_ABOVE, E_LEADING, E_CURRENT, E_LONGEST, E_EPISODES, E_SINCE]] = p
    out[E_ROWS] = rows
    return out


def window_excursions_reference(rows, thresholds) -> np.ndarray:
    """Exact reference, numpy only. ``rows``: ``[n, S]`` float32, oldest first, NaN =
    invalid; ``thresholds``: ``[S, K]`` or ``[K]``. Returns int32 ``[S, K, 8]``. Run lengths
    are the differences of the padded above-mask of the valid samples."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2:
        raise ValueError("rows must be [samples, series]")
    n, S = rows.shape
    t = check_thresholds(thresholds, S)
    out = np.zeros((S, t.shape[1], 8), dtype=np.int32)
    out[:, :, E_ROWS] = n
    for s in range(S):
        x = rows[:, s]
        x = x[~np.isnan(x)]
        out[s, :, E_VALID] = x.size
        for k in range(t.shape[1]):
            above = x > t[s, k]
            edges = np.diff(np.concatenate(([0], above.astype(np.int8), [0])))
            begin, end = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)  # runs [begin, end)
            rec = out[s, k]
            rec[E_ABOVE] = above.sum()
            rec[E_EPISODES] = begin.size
            if begin.size:
                rec[E_LONGEST] = (end - begin).max()
                rec[E_CURRENT] = end[-1] - begin[-1] if end[-1] == x.size else 0
                rec[E_SINCE] = x.size - end[-1]
                rec[E_LEADING] = end[0] if begin[0] == 0 else 0
            else:
                rec[E_SINCE] = x.size
    return out


def excursion_chunk_rows_min(head: int, n: int, depth: int) -> int:
    """The smallest ``chunk_rows`` the chunk cap allows for the window ``[head - n, head)``
    of a ring of ``depth`` rows (each of its one or two blocks is cut on its own)."""
    head, n, depth = int(head), int(n), int(depth)
    first = (head - n) % depth
    rows0 = min(n, depth - first)
    c = max(1, -(-n // MAX_CHUNKS))
    while -(-rows0 // c) + -(-(n - rows0) // c) > MAX_CHUNKS:
        c += 1
    return c


def window_excursions(x, thresholds, head=None, window=None, chunk_rows: int = 0):
    """Run the HIP kernels on a device tensor ``x`` ``[S, n]`` (float32, oldest first, NaN =
    invalid), being rows ``head - n .. head - 1`` (``head`` defaults to n) of a window of
    ``window`` rows (default: the next power of two >= n). The rows are laid into a
    time-major ring of depth ``2 * window`` at their slots - so an arbitrary ``head``
    exercises the wrap - and ``excursion_ring`` runs on the current stream; ``chunk_rows``
    forces that many rows per chunk (0: planned). Returns int32 ``[S, K, 8]`` on the device."""
    import torch

    from ..runtime.native import load

    if not x.is_cuda:
        raise ValueError("window_excursions runs on a GPU tensor; use window_excursions_reference on the CPU")
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    S, n = x.shape
    if not 1 <= S <= MAX_STRIDE:
        raise ValueError(f"1 to {MAX_STRIDE} series in one ring, got {S}")
    if n > MAX_WINDOW:
        raise ValueError(f"window length must be at most {MAX_WINDOW}, got {n}")
    t = check_thresholds(thresholds.detach().cpu().numpy() if isinstance(thresholds, torch.Tensor) else thresholds, S)
    K = t.shape[1]
    if window is None:
        window = 1 << max(0, int(n) - 1).bit_length()
    window = int(window)
    if window < 1 or window & (window - 1):
        raise ValueError(f"window must be a power of two, got {window}")
    head = n if head is None else int(head)
    if not 0 <= n <= min(head, window):
        raise ValueError(f"a window of {n} rows at head {head} (window {window})")
    nat = load()
    depth = 2 * window
    ring = torch.full((depth, S), float("nan"), dtype=torch.float32, device=x.device)
    if n:
        slots = (torch.arange(head - n, head, device=x.device, dtype=torch.int64) % depth)
        ring[slots] = x.to(torch.float32).t()
    td = torch.from_numpy(t).to(x.device)
    work_bytes = nat.excursion_workspace_bytes(S, K)
    work = torch.empty(work_bytes, dtype=torch.uint8, device=x.device)
    out = torch.full((S, K, 8), -1, dtype=torch.int32, device=x.device)
    nat.excursion_ring(ring.data_ptr(), S, S, depth, head, n, td.data_ptr(), K, int(chunk_rows), out.data_ptr(),
                       work.data_ptr(), work_bytes, torch.cuda.current_stream(x.device).cuda_stream)
    return out


def default_thresholds(series, power_limit_w=None, total_vram_mb=None, fractions=(0.5, 0.75, 0.9),
                       card_model=None) -> np.ndarray:
    """[S, K] float32: per series the ``fractions`` of its axis - the axis maximum of
    ``ops.window_buckets.default_bounds`` (its one-bucket bound). 50 / 75 / 90 % are the
    levels the page's share table shows."""
    from .window_buckets import default_bounds

    fr = np.asarray(parse_fractions(fractions), dtype=np.float64)
    axis = default_bounds(series, power_limit_w, total_vram_mb, buckets=1, card_model=card_model)[:, 0].astype(np.float64)
    return check_thresholds(axis[:, None] * fr[None, :])
