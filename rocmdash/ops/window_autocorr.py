"""Window autocorrelation: exact integer lag sums of every series, its correlogram and its
period. HIP entry + exact integer reference.

Kernel: ``csrc/window_autocorr.hip``. Stats, buckets, trend, excursions, heatmap and quantile
trend describe levels, the joint histogram two series at one instant; none describes rhythm.
The telemetry of a training job is periodic - package power, MFMA utilization and HBM bandwidth
rise and fall once per step - so the period is the job's step time read from outside the job,
its strength tells a synchronous job from an irregular one, and the moment it changes tells
when the job slowed down. Prometheus scrapes once a second while the rings run at 10 and 100
Hz: anything faster than 2 s aliases before it arrives. The rows are resident in the device
rings.

Semantics (stated here once; the headers and everything else point here):

* **Span.** For every series ``s`` of a ring, the newest ``N = min(n, span)`` rows of the
  window. ``span`` is a power of two, ``2^6 <= span <= 2^20`` (``MIN_SPAN``, ``MAX_SPAN``),
  default 65536: the work is ``N x (L + 1)`` per series.
* **Quantisation.** An invalid sample (NaN) has ``v[t] = 0`` and ``q[t] = 0``. A valid one has
  ``v[t] = 1`` and ``q[t] = min(max(rint(x * scale[s]), 0), 4095)``: one fp32 multiply, ``rint``
  rounds half to even; ``-inf`` and negatives give 0, ``+inf`` and everything above the axis
  4095. ``scale`` is float32 ``[S]``, finite and positive, by default
  ``float32(4095 / axis[s])`` with the axes of ``default_bucket_bounds``; the host computes it
  once, the reference and the kernel read that same array, the device never divides.
* **Sums.** For lags ``k = 0 .. L``, ``1 <= L <= 1024`` (``MAX_LAGS``), the output is int64
  ``[S][L + 1][4]``, all four over ``0 <= t < N - k`` with ``t = 0`` the oldest row of the span:

  ====== =====================
  word   sum
  ====== =====================
  n_k    sum v[t] v[t + k]
  Sx_k   sum q[t] v[t + k]
  Sy_k   sum v[t] q[t + k]
  Sxy_k  sum q[t] q[t + k]
  ====== =====================

  The kernel works on blocks of 256 lags starting at lag 0, so ``L = 255, 511, 1023`` fill their
  blocks; ``L = 256, 512, 1024`` add a block for the one last lag, whose workgroups stream a chunk
  for a single lag (at ``L = 512`` a third of the workgroups).

  Every word is written, lags ``k >= N`` (all zero) and ``n == 0`` (all zero) included.
  ``Sxy <= 4095^2 x 2^20 < 2^44``: int64 is exact, and the result depends neither on chunking
  nor on the order of combination. ``Sx_0 == Sy_0``; ``n_0`` is the valid count of the span;
  without NaNs ``n_k == N - k`` and ``Sx_k`` / ``Sy_k`` are prefix / suffix sums of ``q``.
* **Correlogram** (host only; Python ints first, one float64 division last). ``var0 = n_0 Sxx_0
  - Sx_0^2`` with ``Sxx_0 = Sxy_0``. If ``n_0 < 2`` or ``var0 <= 0`` the series is constant or
  empty: every ``acf`` is NaN and there is no period. Otherwise ``acf[k] = ((n_k Sxy_k - Sx_k
  Sy_k) / n_k^2) / (var0 / n_0^2)`` where ``2 n_k >= n_0`` and ``n_k > 0``, NaN elsewhere.
* **Period** (host only), ``pick_period(acf, min_strength=0.5, harmonic_tolerance=0.05)``:
  (1) ``k0`` is the first lag ``>= 1`` with ``acf <= 0``; none: no period. (2) Candidates are
  the lags ``k0 < k < L`` whose ``acf[k-1..k+1]`` are all finite with ``acf[k] >= acf[k-1]`` and
  ``acf[k] >= acf[k+1]``. (3) ``M`` is the largest candidate value; ``M < min_strength``: no
  period. (4) The period is the smallest candidate with ``acf >= M - harmonic_tolerance``; its
  ``acf`` is the strength. The two constants are parameters of the definition: the plain
  arg-max returns multiples of the period of a noisy square wave, this rule its period. The
  period is in samples, not seconds, as the excursions' lengths are.

Whole long windows, decimated lags and a spectrum are out of scope; cross-correlation is
``rocmdash.ops.window_xcorr``.

Reference counterpart: none - the reference shows instant values only.
"""

from __future__ import annotations

import numpy as np

from .window_buckets import MAX_LONG_WINDOW, MAX_RING_STRIDE

MAX_LAGS = 1024  # csrc/window_autocorr.h kMaxAutocorrLags
MIN_SPAN = 1 << 6  # kMinAutocorrSpan
MAX_SPAN = 1 << 20  # kMaxAutocorrSpan
DEFAULT_SPAN = 1 << 16
Q_MAX = 4095  # kAutocorrQMax
CHUNK = 1024  # kAutocorrChunk: rows of a kernel chunk (T)
SERIES_GROUP = 8  # series of a workgroup
LAG_BLOCK = 256  # lags of a workgroup
FOLD = 128  # rows an int32 partial of the kernel takes before it is folded into 64 bits
MIN_STRENGTH = 0.5
HARMONIC_TOLERANCE = 0.05


def check_autocorr(L, span=None, window=None) -> tuple:
    """``(L, span)`` as ints (``span`` None: the default): ``ValueError`` unless ``1 <= L <=
    1024``, ``span`` is a power of two in ``[2^6, 2^20]`` and, when a ``window`` is given, ``L``
    is below both the window and the span - a lag the rows cannot reach says nothing."""
    try:
        if isinstance(L, bool) or int(L) != L:
            raise ValueError
        L = int(L)
        span = DEFAULT_SPAN if span is None else span
        if isinstance(span, bool) or int(span) != span:
            raise ValueError
        span = int(span)
    except (TypeError, ValueError):
        raise ValueError(f"lags and span are integers, got {L!r} and {span!r}") from None
    if not 1 <= L <= MAX_LAGS:
        raise ValueError(f"1 to {MAX_LAGS} lags, got {L}")
    if not MIN_SPAN <= span <= MAX_SPAN or span & (span - 1):
        raise ValueError(f"the span is a power of two in [{MIN_SPAN}, {MAX_SPAN}], got {span}")
    if window is not None and L >= min(int(window), span):
        raise ValueError(f"{L} lags need more than {L} rows, the window has {int(window)} and the span {span}")
    return L, span


def parse_autocorr(spec) -> tuple:
    """``"L"`` or ``"L/SPAN"`` (or an ``(L, span)`` pair, or an int) as ``(L, span)``, checked
    by ``check_autocorr``."""
    if isinstance(spec, (tuple, list)) and len(spec) == 2:
        return check_autocorr(spec[0], spec[1])
    if isinstance(spec, (int, np.integer)) and not isinstance(spec, bool):
        return check_autocorr(spec)
    if not isinstance(spec, str):
        raise ValueError(f"a window autocorrelation is 'L' or 'L/SPAN', got {spec!r}")
    ltext, slash, stext = spec.strip().partition("/")
    try:
        L = int(ltext)
        span = int(stext) if slash else None
    except ValueError:
        raise ValueError(f"a window autocorrelation is 'L' or 'L/SPAN' with integers, got {spec!r}") from None
    return check_autocorr(L, span)


def check_scale(scale, num_series: int) -> np.ndarray:
    """``scale`` as contiguous float32 ``[S]`` (a scalar is broadcast), finite and positive."""
    s = np.asarray(scale, dtype=np.float32)
    if s.ndim == 0:
        s = np.full(num_series, s, dtype=np.float32)
    if s.shape != (num_series,):
        raise ValueError(f"scale must be [{num_series}], got {s.shape}")
    if not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("scale must be finite and positive")
    return np.ascontiguousarray(s)


def default_scale(series, power_limit_w=None, total_vram_mb=None, card_model=None) -> np.ndarray:
    """float32 ``[S]``: ``float32(4095 / axis[s])``, the axis maximum of
    ``ops.window_buckets.default_bounds`` (its one-bucket bound)."""
    from .window_buckets import default_bounds

    axis = default_bounds(series, power_limit_w, total_vram_mb, buckets=1, card_model=card_model)[:, 0].astype(np.float64)
    return check_scale((float(Q_MAX) / axis).astype(np.float32), len(axis))


def quantise(rows, scale) -> tuple:
    """``(q, v)`` int64 ``[n, S]`` of float32 rows ``[n, S]``: the quantisation rule above."""
    rows = np.asarray(rows, dtype=np.float32)
    scale = np.asarray(scale, dtype=np.float32)
    v = ~np.isnan(rows)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = rows * scale[None, :]  # one fp32 multiply
        r = np.rint(prod)  # half to even
    q = np.where(v, np.minimum(np.maximum(np.where(v, r, np.float32(0)), np.float32(0)), np.float32(Q_MAX)), np.float32(0))
    return q.astype(np.int64), v.astype(np.int64)


def window_autocorr_reference(rows, scale, L, span=None) -> np.ndarray:
    """Reference, numpy only. ``rows``: ``[n, S]`` float32, the window of one ring, oldest
    first; ``scale``: float32 ``[S]``. Returns int64 ``[S, L + 1, 4]``: the four sums of the
    table above, each written as the table states it."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2:
        raise ValueError("rows must be [samples, series]")
    L, span = check_autocorr(L, span)
    S = rows.shape[1]
    scale = check_scale(scale, S)
    N = min(len(rows), span)
    q, v = quantise(rows[len(rows) - N:], scale)
    out = np.zeros((S, L + 1, 4), dtype=np.int64)
    for k in range(min(L + 1, N)):
        q0, v0, qk, vk = q[: N - k], v[: N - k], q[k:], v[k:]  # [t] and [t + k] over 0 <= t < N - k
        out[:, k, 0] = (v0 * vk).sum(axis=0)
        out[:, k, 1] = (q0 * vk).sum(axis=0)
        out[:, k, 2] = (v0 * qk).sum(axis=0)
        out[:, k, 3] = (q0 * qk).sum(axis=0)
    return out


def correlogram(sums) -> np.ndarray:
    """float64 ``[L + 1]`` (or ``[S, L + 1]`` for ``[S, L + 1, 4]`` sums): the ``acf`` of the
    semantics above, NaN where it is not defined. Python ints, then one float64 division."""
    sums = np.asarray(sums)
    if sums.ndim == 3:
        return np.stack([correlogram(s) for s in sums]) if len(sums) else np.zeros((0, sums.shape[1]))
    if sums.ndim != 2 or sums.shape[1] != 4:
        raise ValueError("sums must be [lags + 1, 4] or [series, lags + 1, 4]")
    acf = np.full(len(sums), np.nan, dtype=np.float64)
    if not len(sums):
        return acf
    n0, sx0, _, sxx0 = (int(x) for x in sums[0])
    var0 = n0 * sxx0 - sx0 * sx0
    if n0 < 2 or var0 <= 0:
        return acf
    for k, (nk, sx, sy, sxy) in enumerate(sums.tolist()):
        if nk > 0 and 2 * nk >= n0:
            acf[k] = ((nk * sxy - sx * sy) * n0 * n0) / (nk * nk * var0)
    return acf


def pick_period(acf, min_strength: float = MIN_STRENGTH, harmonic_tolerance: float = HARMONIC_TOLERANCE) -> tuple:
    """``(period, strength)`` of one series' ``acf`` by the rule above; ``(None, None)`` when
    there is no period."""
    acf = np.asarray(acf, dtype=np.float64)
    L = len(acf) - 1
    with np.errstate(invalid="ignore"):
        down = np.nonzero(acf[1:] <= 0)[0]
    if not len(down):
        return None, None
    k0 = int(down[0]) + 1
    cands = [k for k in range(k0 + 1, L)
             if np.isfinite(acf[k - 1 : k + 2]).all() and acf[k] >= acf[k - 1] and acf[k] >= acf[k + 1]]
    if not cands:
        return None, None
    M = max(acf[k] for k in cands)
    if M < min_strength:
        return None, None
    for k in cands:
        if acf[k] >= M - harmonic_tolerance:
            return k, float(acf[k])
    return None, None


def window_autocorr(x, scale, L, span=None, head=None, window=None, out=None, share=0):
    """Run the HIP kernel on a device tensor ``x`` ``[S, n]`` (float32, oldest first, NaN =
    invalid; one ring of S <= 64 series), being rows ``head - n .. head - 1`` (``head``
    defaults to n) of a window of ``window`` rows (default: the next power of two >= n), with
    ``scale`` ``[S]``, lags ``0 .. L`` and ``span`` (default 65536). The rows are laid into a
    time-major ring of depth ``2 * window`` at their slots, exactly like ``window_joint``, and
    ``autocorr_ring`` runs on the current stream. Returns int64 ``[S, L + 1, 4]`` on the device
    (``out`` when given: a contiguous int64 device tensor of that shape, whatever it holds).
    ``share``: 0 for the launch rule, else the chunks of ``CHUNK`` rows a workgroup takes, ``1 .. max(1, chunks)``."""
    import torch

    from ..runtime.native import load

    if not x.is_cuda:
        raise ValueError("window_autocorr runs on a GPU tensor; use window_autocorr_reference on the CPU")
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    S, n = x.shape
    if not 1 <= S <= MAX_RING_STRIDE:
        raise ValueError(f"1 to {MAX_RING_STRIDE} series in one ring, got {S}")
    if n > MAX_LONG_WINDOW:
        raise ValueError(f"window length must be at most {MAX_LONG_WINDOW}, got {n}")
    L, span = check_autocorr(L, span)
    sc = check_scale(scale.detach().cpu().numpy() if isinstance(scale, torch.Tensor) else scale, S)
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
    sd = torch.from_numpy(sc).to(x.device)
    if out is None:
        out = torch.empty((S, L + 1, 4), dtype=torch.int64, device=x.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (S, L + 1, 4) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"out must be a contiguous int64 [{S}, {L + 1}, 4] tensor on {x.device}")
    load().autocorr_ring(ring.data_ptr(), S, S, depth, head, n, span, sd.data_ptr(), L, out.data_ptr(),
                         torch.cuda.current_stream(x.device).cuda_stream, share=int(share))
    return out
