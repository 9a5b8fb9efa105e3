"""Window cross-correlation: exact integer lead/lag sums of pairs of series, their coefficient
per lag and the lag of a pair. HIP entry + exact integer reference.

Kernel: ``csrc/window_xcorr.hip``. Every other window export describes one series, or - the
joint histogram - two series at the same instant; none says which of two series moves first,
or by how much: does junction temperature follow package power, and after how many samples;
does HBM bandwidth lead or trail MFMA utilization within a training step; does power still
follow activity (a vanished or inverted coupling is a throttled card). Prometheus scrapes once
a second while the rings run at 10 and 100 Hz: the pairing of rows and every lag under a
second are lost before the data arrives. The rows are resident in the device rings.

Semantics (stated here once; the headers and everything else point here):

* **Pairs.** 1 to 8 (``MAX_PAIRS``) ordered pairs ``(a, b)`` of series indices, ``a != b``, both
  of the same ring: ``rocmdash.ops.window_joint.check_pairs``, unchanged, its refusal of a
  cross-ring pair included. A series may appear in several pairs.
* **Span and quantisation** are exactly the autocorrelation's
  (``rocmdash.ops.window_autocorr``): the newest ``N = min(n, span)`` rows, ``span`` a power of
  two in ``2^6 .. 2^20``, default 65536; ``q``, ``v`` and ``scale[S]`` are its ``quantise``,
  ``check_scale`` and ``default_scale``.
* **Lags.** ``k = -L .. L``, ``1 <= L <= 1024``. Lag ``k`` pairs ``a[t]`` with ``b[t + k]`` over
  all ``t`` with ``0 <= t < N`` and ``0 <= t + k < N``; ``t = 0`` is the oldest row of the span.
  A peak at ``k > 0`` means ``b`` follows ``a`` by ``k`` samples.
* **Sums.** The output is int64 ``[K][2L + 1][6]``, lag ``k`` at index ``L + k``:

  ====== ==========================
  word   sum
  ====== ==========================
  n      sum va[t] vb[t + k]
  Sx     sum qa[t] vb[t + k]
  Sy     sum va[t] qb[t + k]
  Sxy    sum qa[t] qb[t + k]
  Sxx    sum qa[t]^2 vb[t + k]
  Syy    sum va[t] qb[t + k]^2
  ====== ==========================

  Every word is written, lags with ``|k| >= N`` (all zero) and empty windows (all zero)
  included. Every word is ``<= 4095^2 x 2^20 < 2^44``: int64 is exact, and the result depends
  neither on chunking nor on the order of combination.
* **Identities.** ``(b, a)`` at lag ``k`` is ``(a, b)`` at lag ``-k`` with ``Sx <-> Sy`` and
  ``Sxx <-> Syy``. Without NaNs ``n_k = N - |k|``.
* **Cross-correlogram** (host only), ``cross_correlogram(sums)``: float64 ``[2L + 1]``, the
  Pearson coefficient per lag over the samples that pair up. With Python ints ``num = n Sxy - Sx
  Sy``, ``da = n Sxx - Sx^2``, ``db = n Syy - Sy^2``; ``r_k = num / sqrt(da db)`` with one float64
  square root and one division last. ``r_k`` is NaN where ``n_k < 2``, where ``2 n_k < n_0``, or
  where ``da <= 0`` or ``db <= 0``. It is clipped to ``[-1, 1]`` only against the final rounding.
* **Lag** (host only), ``pick_lag(ccf, min_strength=0.5, tolerance=0.05)``: (1) candidates are
  the lags ``-L < k < L`` whose ``|r|`` at ``k - 1``, ``k`` and ``k + 1`` are all finite with
  ``|r_k| >= |r_{k-1}|`` and ``|r_k| >= |r_{k+1}|``; the ends ``+-L`` are never candidates, because
  a peak there may lie outside the range. (2) ``M`` is the largest candidate ``|r|``; ``M <
  min_strength``: no lag. (3) The lag is the candidate with the smallest ``|k|`` among those with
  ``|r| >= M - tolerance``; a tie between ``+k`` and ``-k`` goes to the larger ``|r|``, then to
  ``+k``. The returned ``r`` is signed. The two constants are parameters of the definition, as
  ``pick_period``'s are: a periodic pair has near-equal peaks one period apart, the plain
  arg-max picks any of them, this rule the one nearest zero. The lag is in samples, not
  seconds.

The rank-per-GPU service, ``snapshot_io``, cross-ring pairs, a node-merged result, lags in
seconds, spans above 2^20 and any resident or incremental state are out of scope.

Reference counterpart: none - the reference shows instant values only.
"""

from __future__ import annotations

import math

import numpy as np

from .window_autocorr import (DEFAULT_SPAN, MAX_LAGS, check_autocorr, check_scale, default_scale,  # noqa: F401
                              quantise)
from .window_buckets import MAX_LONG_WINDOW, MAX_RING_STRIDE
from .window_joint import DEFAULT_PAIRS, MAX_PAIRS, check_pairs, parse_joint  # noqa: F401

WORDS = 6  # csrc/window_xcorr_plan.h kXcorrWords: n, Sx, Sy, Sxy, Sxx, Syy
GROUP_PAIRS = 4  # kXcorrGroupPairs: pairs of a workgroup
LAG_BLOCK = 256  # kXcorrLagBlock: lags of a workgroup
LAG_TILE = 8  # kXcorrLagTile: lags of a thread
DEFAULT_LAGS = 255  # lags 0 .. 255 fill exactly one block of 256 lags; 256 would add a block for one lag
MIN_STRENGTH = 0.5
TOLERANCE = 0.05


def check_xcorr(L, span=None, window=None) -> tuple:
    """``(L, span)`` as ints: the autocorrelation's refusals (``check_autocorr``), ``L >=
    min(window, span)`` included when a ``window`` is given."""
    return check_autocorr(L, span, window)


def parse_xcorr(spec, series, widths=None) -> tuple:
    """``PAIRS[/L[/SPAN]]`` as ``(pairs, L, span)``. ``PAIRS`` is exactly ``parse_joint``'s pair
    syntax - ``default`` (those of ``window_joint.DEFAULT_PAIRS`` whose two series exist) or
    ``metricA:metricB,metricC:metricD``, the ``amd_gpu_`` prefix optional - and is parsed by it;
    ``L`` defaults to 255 and ``SPAN`` to 65536, both checked by ``check_xcorr``."""
    if not isinstance(spec, str):
        raise ValueError(f"a window cross-correlation is 'default' or 'metricA:metricB,..' with an optional /L/SPAN, got {spec!r}")
    parts = spec.strip().split("/")
    if len(parts) > 3:
        raise ValueError(f"a window cross-correlation is PAIRS[/L[/SPAN]], got {spec!r}")
    try:
        L = int(parts[1]) if len(parts) > 1 else DEFAULT_LAGS
        span = int(parts[2]) if len(parts) > 2 else None
    except ValueError:
        raise ValueError(f"the lags and the span after '/' must be integers, got {spec!r}") from None
    pairs, _ = parse_joint(parts[0], series, widths)
    L, span = check_xcorr(L, span)
    return pairs, L, span


def window_xcorr_reference(rows, pairs, scale, L, span=None) -> np.ndarray:
    """Reference, numpy only. ``rows``: ``[n, S]`` float32, the window of one ring (or of a set
    whose pairs were checked by ``check_pairs``), oldest first; ``pairs``: ``[(a, b), ..]``;
    ``scale``: float32 ``[S]``. Returns int64 ``[K, 2L + 1, 6]``: the six sums of the table
    above, each written as the table states it."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2:
        raise ValueError("rows must be [samples, series]")
    L, span = check_xcorr(L, span)
    S = rows.shape[1]
    scale = check_scale(scale, S)
    pairs = check_pairs(pairs, S)
    N = min(len(rows), span)
    q, v = quantise(rows[len(rows) - N:], scale)
    out = np.zeros((len(pairs), 2 * L + 1, WORDS), dtype=np.int64)
    for i, (a, b) in enumerate(pairs):
        for k in range(-L, L + 1):
            if abs(k) >= N:
                continue
            t0, t1 = max(0, -k), min(N, N - k)  # 0 <= t < N and 0 <= t + k < N
            qa, va, qb, vb = q[t0:t1, a], v[t0:t1, a], q[t0 + k : t1 + k, b], v[t0 + k : t1 + k, b]
            out[i, L + k, 0] = (va * vb).sum()
            out[i, L + k, 1] = (qa * vb).sum()
            out[i, L + k, 2] = (va * qb).sum()
            out[i, L + k, 3] = (qa * qb).sum()
            out[i, L + k, 4] = (qa * qa * vb).sum()
            out[i, L + k, 5] = (va * qb * qb).sum()
    return out


def cross_correlogram(sums) -> np.ndarray:
    """float64 ``[2L + 1]`` (or ``[K, 2L + 1]`` for ``[K, 2L + 1, 6]`` sums): the ``r_k`` of the
    semantics above, NaN where it is not defined. Python ints, then one float64 square root and
    one division."""
    sums = np.asarray(sums)
    if sums.ndim == 3:
        return np.stack([cross_correlogram(s) for s in sums]) if len(sums) else np.zeros((0, sums.shape[1]))
    if sums.ndim != 2 or sums.shape[1] != WORDS or len(sums) % 2 != 1:
        raise ValueError("sums must be [2 lags + 1, 6] or [pairs, 2 lags + 1, 6]")
    ccf = np.full(len(sums), np.nan, dtype=np.float64)
    n0 = int(sums[len(sums) // 2, 0])
    for i, (n, sx, sy, sxy, sxx, syy) in enumerate(sums.tolist()):
        if n < 2 or 2 * n < n0:
            continue
        num, da, db = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
        if da <= 0 or db <= 0:
            continue
        ccf[i] = min(1.0, max(-1.0, num / math.sqrt(da * db)))
    return ccf


def pick_lag(ccf, min_strength: float = MIN_STRENGTH, tolerance: float = TOLERANCE) -> tuple:
    """``(lag, r)`` of one pair's ``ccf`` ``[2L + 1]`` by the rule above, ``r`` signed;
    ``(None, None)`` when there is no lag."""
    ccf = np.asarray(ccf, dtype=np.float64)
    if ccf.ndim != 1 or len(ccf) % 2 != 1:
        raise ValueError("ccf must be [2 lags + 1]")
    L = len(ccf) // 2
    mag = np.abs(ccf)
    cands = [k for k in range(-L + 1, L)
             if np.isfinite(mag[L + k - 1 : L + k + 2]).all() and mag[L + k] >= mag[L + k - 1] and mag[L + k] >= mag[L + k + 1]]
    if not cands:
        return None, None
    M = max(mag[L + k] for k in cands)
    if M < min_strength:
        return None, None
    near = [k for k in cands if mag[L + k] >= M - tolerance]
    k = min(near, key=lambda k: (abs(k), -mag[L + k], -k))  # smallest |k|, then the larger |r|, then +k
    return k, float(ccf[L + k])


def window_xcorr(x, pairs, scale, L, span=None, head=None, window=None, out=None, share=0):
    """Run the HIP kernel on a device tensor ``x`` ``[S, n]`` (float32, oldest first, NaN =
    invalid; one ring of S <= 64 series), being rows ``head - n .. head - 1`` (``head``
    defaults to n) of a window of ``window`` rows (default: the next power of two >= n), with
    ``pairs``, ``scale`` ``[S]``, lags ``-L .. L`` and ``span`` (default 65536). The rows are
    laid into a time-major ring of depth ``2 * window`` at their slots, exactly like
    ``window_autocorr``, and ``xcorr_ring`` runs on the current stream. Returns int64 ``[K, 2L +
    1, 6]`` on the device (``out`` when given: a contiguous int64 device tensor of that shape,
    whatever it holds). ``share``: 0 for the launch rule, else the chunks a workgroup takes, as ``window_autocorr``'s."""
    import torch

    from ..runtime.native import load

    if not x.is_cuda:
        raise ValueError("window_xcorr runs on a GPU tensor; use window_xcorr_reference on the CPU")
    if x.ndim != 2:
        raise ValueError("x must be [series, samples]")
    S, n = x.shape
    if not 1 <= S <= MAX_RING_STRIDE:
        raise ValueError(f"1 to {MAX_RING_STRIDE} series in one ring, got {S}")
    if n > MAX_LONG_WINDOW:
        raise ValueError(f"window length must be at most {MAX_LONG_WINDOW}, got {n}")
    L, span = check_xcorr(L, span)
    sc = check_scale(scale.detach().cpu().numpy() if isinstance(scale, torch.Tensor) else scale, S)
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
    sd = torch.from_numpy(sc).to(x.device)
    shape = (len(pairs), 2 * L + 1, WORDS)
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=x.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"out must be a contiguous int64 {list(shape)} tensor on {x.device}")
    load().xcorr_ring(ring.data_ptr(), S, S, depth, head, n, span, sd.data_ptr(), pairs, L, out.data_ptr(),
                      torch.cuda.current_stream(x.device).cuda_stream, share=int(share))
    return out
