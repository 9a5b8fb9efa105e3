"""Node exporter: ``/metrics`` with the ``amd_gpu_*`` series the dashboard queries.

Reference counterpart: the AMD device-metrics exporter the reference assumes is
scraped by Prometheus (``app.py:168-171``; not part of the reference repo). This
exporter is fed by rocmdash's own native pipeline:

  * ``LocalNodeSource``: the single-process exporter (no torchrun): one ``GpuAgent``
    per device with background native samplers (amd-smi 10 Hz, device counters
    100 Hz); a scrape refreshes every agent's device window (one window-stats launch
    per GPU) and renders latest values + per-GPU window statistics. It does no
    node-wide aggregation: the node-window statistics and the whole-node tensor come
    only from the rank-per-GPU service (``rocmdash.serve``, RCCL all-gather), the one
    node-aggregation path;
  * ``PipelineSource``: rank 0 of the rank-per-GPU pipeline (``rocmdash.serve``)
    renders the RCCL-gathered node snapshot;
  * ``SyntheticSource``: a synthetic node (CPU tests, demos).

Every scrape also reports the exporter's own health: sampler counts/failures/
overruns, last sample age (staleness), scrape and refresh durations.

    python -m rocmdash.prom.exporter --port 9400            # all local GPUs
    python -m rocmdash.prom.exporter --synthetic 8 --port 9400
"""

from __future__ import annotations

import argparse
import json
import logging
import os
import socket
import threading
import time
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

import numpy as np

from ..models.health import SourceHealth
from ..models.schema import HEALTH_SOURCES, STAT_INDEX
from ..utils.timing import LatencyHistogram
from ..viz.panels import NodeSnapshot
from .exposition import Exposition, render_snapshot

log = logging.getLogger("rocmdash.prom.exporter")
CONTENT_TYPE = "text/plain; version=0.0.4; charset=utf-8"
LAST = STAT_INDEX["last"]


def node_bucket_sum(buckets: np.ndarray) -> np.ndarray:
    """The node's le-buckets: per-GPU counts ``[N, S, B + 1]`` summed over the GPUs in
    float64, in the dtype of the counts - float32 for short windows (N x 32768 < 2^24),
    float64 for long ones, whose sums pass 2^24."""
    return buckets.sum(axis=0, dtype=np.float64).astype(buckets.dtype)


class SnapshotSource:
    """Produces (NodeSnapshot, self_metrics: Exposition) per scrape."""

    def collect(self):  # pragma: no cover - interface
        raise NotImplementedError

    def close(self) -> None:
        pass


class SyntheticSource(SnapshotSource):
    def __init__(self, n_gpus: int = 8, seed: int = 0):
        from .mock import SyntheticNode

        self.node = SyntheticNode(n_gpus, seed=seed)

    def collect(self):
        self.node.step()
        cols = None
        rows = []
        for g in range(len(self.node.gpu_ids)):
            v = self.node.values(g)
            cols = tuple(v)
            rows.append([v[c] for c in cols])
        snap = NodeSnapshot(
            gpu_ids=list(self.node.gpu_ids),
            card_models=[self.node.card_model] * len(rows),
            columns=cols,
            values=rows,
        )
        return snap, None


class LocalNodeSource(SnapshotSource):
    """Every visible GPU in this process, background sampling, stats per scrape."""

    def __init__(self, devices=None, source: str = "auto", counters: str = "auto", cfg=None,
                 window_buckets: int | None = None, window_trend: int | None = None, window_excursions=None,
                 replay=None, window_heatmap=None, window_joint=None, window_quantiles: int | None = None,
                 window_autocorr=None, window_xcorr=None, window_periods=None):
        """``window_buckets`` = B > 0 (default: ``ROCMDASH_WINDOW_BUCKETS``, else off): also
        export every series' window as B cumulative le-buckets + ``+Inf``
        (``rocmdash_window_bucket``; GpuAgent.window_buckets) and their sum over the GPUs -
        short windows as float32 counts, long windows (> 32768 samples) as float64.
        ``window_trend`` = P > 0 (default: ``ROCMDASH_WINDOW_TREND``, else off): the snapshot
        also carries every series' window as P + 1 columns of {min, max, mean, count}
        (GpuAgent.window_trend), served as JSON by ``GET /trend`` - never in ``/metrics``.
        ``window_excursions`` = ``"F1,F2,.."`` or a sequence of 1 to 4 increasing fractions in
        (0, 1] (default: ``ROCMDASH_WINDOW_EXCURSIONS``, else off): also export every series'
        episodes above those fractions of its axis (``rocmdash_window_excursions`` and its
        neighbours; GpuAgent.window_excursions). ``replay``: the recording of ``source="replay"``.
        ``window_heatmap`` = ``"PxB"`` or ``(P, B)`` (default: ``ROCMDASH_WINDOW_HEATMAP``, else
        off): the snapshot also carries every series' window as P + 1 columns of B + 1 bin
        counts (GpuAgent.window_heatmap), served as JSON by ``GET /heatmap`` - never in
        ``/metrics``. ``window_joint`` = ``"default"`` or ``"metricA:metricB,.."`` with an
        optional ``/B`` (``rocmdash.ops.window_joint.parse_joint``; default:
        ``ROCMDASH_WINDOW_JOINT``, else off): the snapshot also carries the joint histograms of
        those pairs of series (GpuAgent.window_joint), served as JSON by ``GET /joint`` - never
        in ``/metrics``. ``window_quantiles`` = P > 0 (default: ``ROCMDASH_WINDOW_QUANTILES``,
        else off): the snapshot also carries every series' window as P + 1 columns of its three
        percentiles and their count (GpuAgent.window_quantiles), served as JSON by
        ``GET /quantiles`` - never in ``/metrics``. ``window_autocorr`` = ``"L"`` or ``"L/SPAN"``
        (``rocmdash.ops.window_autocorr.parse_autocorr``; default: ``ROCMDASH_WINDOW_AUTOCORR``, else
        off): the snapshot also carries every series' autocorrelation sums
        (GpuAgent.window_autocorr), served as JSON by ``GET /autocorr``, and ``/metrics`` gains
        ``rocmdash_window_period_samples`` / ``_strength`` for the series that have a period.
        ``window_xcorr`` = ``"PAIRS[/L[/SPAN]]"`` (``rocmdash.ops.window_xcorr.parse_xcorr``; default:
        ``ROCMDASH_WINDOW_XCORR``, else off): the snapshot also carries the cross-correlation sums of
        those pairs (GpuAgent.window_xcorr), served as JSON by ``GET /xcorr``, and ``/metrics`` gains
        ``rocmdash_window_lag_samples`` / ``_correlation`` for the pairs that have a lag.
        ``window_periods`` = ``"P[/L[/SPAN]]"`` (``rocmdash.ops.window_periods.parse_periods``; default:
        ``ROCMDASH_WINDOW_PERIODS``, else off): the snapshot also carries every series' autocorrelation
        sums per trend column of the newest SPAN rows (GpuAgent.window_periods), served as JSON by
        ``GET /periods`` - never in ``/metrics``."""
        from ..runtime import native

        if window_excursions is None:
            window_excursions = os.environ.get("ROCMDASH_WINDOW_EXCURSIONS", "") or None
        self.excursion_fractions = None
        if window_excursions is not None:  # checked before any agent starts its samplers
            from ..ops.window_excursions import parse_fractions

            self.excursion_fractions = parse_fractions(window_excursions)

        if window_trend is None:
            window_trend = int(os.environ.get("ROCMDASH_WINDOW_TREND", "0") or 0)
        self.trend_columns = int(window_trend) if window_trend else None
        if self.trend_columns is not None:  # checked before any agent starts its samplers
            from ..config import SamplerConfig
            from ..ops.window_trend import check_columns

            check_columns(self.trend_columns, (cfg or SamplerConfig()).window)
        if window_quantiles is None:
            window_quantiles = int(os.environ.get("ROCMDASH_WINDOW_QUANTILES", "0") or 0)
        self.quantile_columns = int(window_quantiles) if window_quantiles else None
        if self.quantile_columns is not None:  # checked before any agent starts its samplers
            from ..config import SamplerConfig
            from ..ops.window_quantiles import check_columns

            check_columns(self.quantile_columns, (cfg or SamplerConfig()).window)
        if window_heatmap is None:
            window_heatmap = os.environ.get("ROCMDASH_WINDOW_HEATMAP", "") or None
        self.heatmap = None
        if window_heatmap is not None:  # checked before any agent starts its samplers
            from ..config import SamplerConfig
            from ..ops.window_heatmap import parse_heatmap
            from ..ops.window_trend import check_columns

            self.heatmap = parse_heatmap(window_heatmap)
            check_columns(self.heatmap[0], (cfg or SamplerConfig()).window)
        if window_autocorr is None:
            window_autocorr = os.environ.get("ROCMDASH_WINDOW_AUTOCORR", "") or None
        self.autocorr = None  # (L, span): rocmdash.ops.window_autocorr; GET /autocorr and the two period gauges
        if window_autocorr is not None:  # checked before any agent starts its samplers
            from ..config import SamplerConfig
            from ..ops.window_autocorr import check_autocorr, parse_autocorr

            self.autocorr = check_autocorr(*parse_autocorr(window_autocorr), (cfg or SamplerConfig()).window)
        if window_periods is None:
            window_periods = os.environ.get("ROCMDASH_WINDOW_PERIODS", "") or None
        self.periods = None  # (P, L, span): rocmdash.ops.window_periods; GET /periods
        if window_periods is not None:  # checked before any agent starts its samplers
            from ..config import SamplerConfig
            from ..ops.window_periods import parse_periods

            self.periods = parse_periods(window_periods, (cfg or SamplerConfig()).window)
        if window_joint is None:
            window_joint = os.environ.get("ROCMDASH_WINDOW_JOINT", "") or None
        if window_joint is not None:  # the spec, its metrics and its rings: checked before any agent exists
            from ..models.schema import CTR_FIELDS, SMI_FIELDS
            from ..ops.window_joint import parse_joint

            parse_joint(window_joint, SMI_FIELDS + CTR_FIELDS, (len(SMI_FIELDS), len(CTR_FIELDS)))
        if window_xcorr is None:
            window_xcorr = os.environ.get("ROCMDASH_WINDOW_XCORR", "") or None
        if window_xcorr is not None:  # the spec, its metrics, its rings and its lags: checked before any agent exists
            from ..config import SamplerConfig
            from ..models.schema import CTR_FIELDS, SMI_FIELDS
            from ..ops.window_xcorr import check_xcorr, parse_xcorr

            _, xl, xs = parse_xcorr(window_xcorr, SMI_FIELDS + CTR_FIELDS, (len(SMI_FIELDS), len(CTR_FIELDS)))
            check_xcorr(xl, xs, (cfg or SamplerConfig()).window)
        native.load()
        if counters in ("auto", "hw"):
            native.enable_counters()
        import torch

        from ..runtime.agent import GpuAgent

        n = torch.cuda.device_count() if torch.cuda.is_available() else 0
        devices = list(range(n)) if devices is None else list(devices)
        if not devices:
            raise RuntimeError("no GPU visible to the exporter (use --synthetic N for a synthetic node)")
        kw = {"replay": replay} if replay is not None else {}
        self.agents = [GpuAgent(d, source=source, counters=counters, cfg=cfg, **kw) for d in devices]
        series = {a.series for a in self.agents}
        if len(series) != 1:
            raise RuntimeError(f"GPUs disagree on the series layout: {series}")
        self.series = self.agents[0].series
        self.joint = None  # (pairs, B): against the series these GPUs have, still before any sampler starts
        if window_joint is not None:
            from ..ops.window_joint import parse_joint

            try:
                self.joint = parse_joint(window_joint, self.series, [r.width for r in self.agents[0].rings])
            except ValueError:
                self.close()
                raise
        self.xcorr = None  # (pairs, L, span): rocmdash.ops.window_xcorr; GET /xcorr and the two lag gauges
        if window_xcorr is not None:
            from ..ops.window_xcorr import parse_xcorr

            try:
                self.xcorr = parse_xcorr(window_xcorr, self.series, [r.width for r in self.agents[0].rings])
            except ValueError:
                self.close()
                raise
        for a in self.agents:
            a.start()
        self._lock = threading.Lock()
        self.last_refresh_s = 0.0
        self.refresh_hist = LatencyHistogram("rocmdash_refresh_latency_seconds", "Device refresh latency per scrape")
        self._health = np.empty((len(self.agents), len(HEALTH_SOURCES), 8), dtype=np.float32)
        if window_buckets is None:
            window_buckets = int(os.environ.get("ROCMDASH_WINDOW_BUCKETS", "0") or 0)
        # one set of bounds for the node (the first GPU's caps): buckets add up only over the same bounds
        self.bucket_bounds = self.agents[0].default_bucket_bounds(int(window_buckets)) if window_buckets else None
        # likewise one set of thresholds for the node
        self.excursion_thresholds = (self.agents[0].default_excursion_thresholds(self.excursion_fractions)
                                     if self.excursion_fractions else None)
        # and one set of heatmap bounds
        self.heatmap_bounds = self.agents[0].default_bucket_bounds(self.heatmap[1]) if self.heatmap else None
        # and one set of joint bounds
        self.joint_bounds = self.agents[0].default_bucket_bounds(self.joint[1]) if self.joint else None
        # and one autocorrelation scale
        self.autocorr_scale = self.agents[0].default_autocorr_scale() if self.autocorr else None
        # the cross-correlation quantises by the same rule
        self.xcorr_scale = self.agents[0].default_autocorr_scale() if self.xcorr else None
        # and so does the period trend
        self.periods_scale = self.agents[0].default_autocorr_scale() if self.periods else None

    def collect(self):
        import torch

        with self._lock:
            t0 = time.perf_counter()
            outs = [a.refresh() for a in self.agents]  # one launch per GPU, all async
            buckets = None
            if self.bucket_bounds is not None:  # in stream order behind each GPU's refresh
                buckets = [a.window_buckets(self.bucket_bounds) for a in self.agents]
            trend = age = None
            if self.trend_columns is not None:  # likewise: the rings as this refresh left them
                trend = [a.window_trend(self.trend_columns) for a in self.agents]
                age = self.agents[0].trend_age_rows(self.trend_columns)
            excursions = None
            if self.excursion_thresholds is not None:
                excursions = [a.window_excursions(self.excursion_thresholds) for a in self.agents]
            heatmap = heat_age = None
            if self.heatmap is not None:
                heatmap = [a.window_heatmap(self.heatmap[0], self.heatmap_bounds) for a in self.agents]
                heat_age = self.agents[0].trend_age_rows(self.heatmap[0])
            joint = None
            if self.joint is not None:
                joint = [a.window_joint(self.joint[0], self.joint_bounds) for a in self.agents]
            autocorr = None
            if self.autocorr is not None:
                autocorr = [a.window_autocorr(self.autocorr[0], self.autocorr[1], self.autocorr_scale) for a in self.agents]
            xcorr = None
            if self.xcorr is not None:
                xcorr = [a.window_xcorr(self.xcorr[0], self.xcorr[1], self.xcorr[2], self.xcorr_scale) for a in self.agents]
            periods = periods_age = None
            if self.periods is not None:
                periods = [a.window_periods(self.periods[0], self.periods[1], self.periods[2], self.periods_scale)
                           for a in self.agents]
                periods_age = self.agents[0].periods_age_rows(self.periods[0], self.periods[2])
            quantiles = quant_age = None
            if self.quantile_columns is not None:
                quantiles = [a.window_quantiles(self.quantile_columns) for a in self.agents]
                quant_age = self.agents[0].trend_age_rows(self.quantile_columns)
            host = np.stack([o.to("cpu", non_blocking=False).numpy() for o in outs])
            if buckets is not None:
                buckets = np.stack([b.to("cpu", non_blocking=False).numpy() for b in buckets])
            if trend is not None:
                trend = np.stack([t.to("cpu", non_blocking=False).numpy() for t in trend])
            if excursions is not None:
                excursions = np.stack([e.to("cpu", non_blocking=False).numpy() for e in excursions])
            if heatmap is not None:
                heatmap = np.stack([h.to("cpu", non_blocking=False).numpy() for h in heatmap])
            if joint is not None:
                joint = np.stack([j.to("cpu", non_blocking=False).numpy() for j in joint])
            if autocorr is not None:
                autocorr = np.stack([c.to("cpu", non_blocking=False).numpy() for c in autocorr])
            if xcorr is not None:
                xcorr = np.stack([c.to("cpu", non_blocking=False).numpy() for c in xcorr])
            if periods is not None:
                periods = np.stack([c.to("cpu", non_blocking=False).numpy() for c in periods])
            if quantiles is not None:
                quantiles = np.stack([q.to("cpu", non_blocking=False).numpy() for q in quantiles])
            now_ns = time.time_ns()
            for i, a in enumerate(self.agents):
                a.health_rows(self._health[i], now_ns)
            self.last_refresh_s = time.perf_counter() - t0
            self.refresh_hist.observe(self.last_refresh_s)
        ids = [a.info.gpu_id for a in self.agents]
        if len(set(ids)) != len(ids):
            ids = [str(a.device_index) for a in self.agents]
        snap = NodeSnapshot(
            gpu_ids=ids,
            card_models=[a.info.card_model for a in self.agents],
            columns=self.series,
            values=host[:, :, LAST],
            power_limits=[a.info.power_limit_w for a in self.agents],
            product_names=[a.info.product_name for a in self.agents],
            window=host,
            window_series=self.series,
            xcd=np.stack([a.xcd() for a in self.agents]),
            # same per-source health rows the rank-per-GPU service gathers
            source_health=SourceHealth(self._health.copy(),
                                       [(a.info.smi_backend, a.info.counter_backend) for a in self.agents],
                                       self.agents[0].cfg.stale_periods),
        )
        if buckets is not None:
            snap.window_buckets = buckets
            snap.window_bucket_bounds = self.bucket_bounds
            snap.node_window_buckets = node_bucket_sum(buckets)
        if trend is not None:
            snap.window_trend, snap.window_trend_age_rows = trend, age
        if excursions is not None:
            snap.window_excursions, snap.window_excursion_thresholds = excursions, self.excursion_thresholds
        if heatmap is not None:
            snap.window_heatmap, snap.window_heatmap_age_rows = heatmap, heat_age
            snap.window_heatmap_bounds = np.broadcast_to(self.heatmap_bounds, (len(ids),) + self.heatmap_bounds.shape)
        if joint is not None:
            snap.window_joint, snap.window_joint_pairs = joint, tuple(self.joint[0])
            snap.window_joint_bounds = np.broadcast_to(self.joint_bounds, (len(ids),) + self.joint_bounds.shape)
        if autocorr is not None:
            snap.window_autocorr, snap.window_autocorr_span = autocorr, self.autocorr[1]
        if xcorr is not None:
            snap.window_xcorr, snap.window_xcorr_pairs, snap.window_xcorr_span = xcorr, tuple(self.xcorr[0]), self.xcorr[2]
        if periods is not None:
            snap.window_periods, snap.window_periods_span, snap.window_periods_age_rows = periods, self.periods[2], periods_age
        if quantiles is not None:
            snap.window_quantiles, snap.window_quantiles_age_rows = quantiles, quant_age
            snap.window_quantiles_pct = tuple(self.agents[0].pct)
        exp = Exposition()
        for a, gid in zip(self.agents, ids):
            for sampler in a.samplers:
                lab = {"gpu_id": gid, "source": sampler.source.kind, "backend": sampler.source.backend}
                exp.add("rocmdash_sampler_read_seconds", sampler.stats()["mean_us"] * 1e-6, lab,
                        "Mean duration of one source read")
        exp.add("rocmdash_refresh_seconds", self.last_refresh_s, {}, "Device refresh (stats kernel + D2H) of the last scrape")
        self.refresh_hist.add_to(exp)
        if any(a.use_gpu for a in self.agents):
            torch.cuda.synchronize()
        return snap, exp

    def close(self) -> None:
        for a in self.agents:
            a.close()


class PipelineSource(SnapshotSource):
    """Rank 0 of ``NodePipeline`` (background sampling on every rank)."""

    def __init__(self, pipeline):
        self.pipeline = pipeline
        self._lock = threading.Lock()

    def collect(self):
        with self._lock:
            return self.pipeline.latest_snapshot(), None


def _nullable(x) -> list:
    """A float array as a JSON-ready list: NaN becomes None (JSON has no NaN)."""
    return [None if v != v else float(v) for v in np.asarray(x, dtype=np.float64).ravel()]


def render_trend(snap: NodeSnapshot) -> str | None:
    """The snapshot's window trend as the ``/trend`` document, None when it carries none:
    ``{"columns": P, "age_rows": [P + 1], "series": [...], "gpus": {gpu_id: {metric: {"min":
    [P + 1], "max": ..., "mean": ..., "count": ...}}}}``, slot 0 the oldest, empty slots null."""
    trend = getattr(snap, "window_trend", None)
    if trend is None:
        return None
    trend = np.asarray(trend)
    series = list(snap.window_series)
    gpus = {}
    for g, gid in enumerate(snap.gpu_ids):
        gpus[gid] = {m: {k: _nullable(trend[g, s, :, i]) for i, k in enumerate(("min", "max", "mean", "count"))}
                     for s, m in enumerate(series)}
    age = snap.window_trend_age_rows
    doc = {"columns": int(trend.shape[2]) - 1, "age_rows": _nullable(age) if age is not None else None,
           "series": series, "gpus": gpus}
    return json.dumps(doc, allow_nan=False)


def quantile_keys(pct) -> list:
    """The ``/quantiles`` document's key of each percentile: ``p50``, ``p99.9``."""
    return [f"p{float(p):g}" for p in pct]


def render_quantiles(snap: NodeSnapshot) -> str | None:
    """The snapshot's window quantile trend as the ``/quantiles`` document, None when it carries
    none: ``{"columns": P, "percentiles": [a, b, c], "age_rows": [P + 1], "series": [...],
    "gpus": {gpu_id: {metric: {"p<a>": [P + 1], "p<b>": ..., "p<c>": ..., "count": ...}}}}``,
    slot 0 the oldest, empty slots null."""
    quant = getattr(snap, "window_quantiles", None)
    pct = getattr(snap, "window_quantiles_pct", None)
    if quant is None or pct is None:
        return None
    quant = np.asarray(quant)
    series = list(snap.window_series)
    keys = quantile_keys(pct) + ["count"]
    gpus = {}
    for g, gid in enumerate(snap.gpu_ids):
        gpus[gid] = {m: {k: _nullable(quant[g, s, :, i]) for i, k in enumerate(keys)} for s, m in enumerate(series)}
    age = getattr(snap, "window_quantiles_age_rows", None)
    doc = {"columns": int(quant.shape[2]) - 1, "percentiles": [float(p) for p in pct],
           "age_rows": _nullable(age) if age is not None else None, "series": series, "gpus": gpus}
    return json.dumps(doc, allow_nan=False)


def render_heatmap(snap: NodeSnapshot) -> str | None:
    """The snapshot's window heatmap as the ``/heatmap`` document, None when it carries none:
    ``{"columns": P, "buckets": B, "age_rows": [P + 1], "series": [...], "gpus": {gpu_id:
    {metric: {"le": [B bounds], "counts": [[B + 1 ints] x (P + 1)]}}}}``, slot 0 the oldest;
    counts are per bin (not cumulative), the last bin being everything above the last bound."""
    heat = getattr(snap, "window_heatmap", None)
    bounds = getattr(snap, "window_heatmap_bounds", None)
    if heat is None or bounds is None:
        return None
    heat, bounds = np.asarray(heat), np.asarray(bounds)
    series = list(snap.window_series)
    gpus = {}
    for g, gid in enumerate(snap.gpu_ids):
        gpus[gid] = {m: {"le": [float(v) for v in bounds[g, s]], "counts": heat[g, s].tolist()}
                     for s, m in enumerate(series)}
    age = getattr(snap, "window_heatmap_age_rows", None)
    doc = {"columns": int(heat.shape[2]) - 1, "buckets": int(heat.shape[3]) - 1,
           "age_rows": _nullable(age) if age is not None else None, "series": series, "gpus": gpus}
    return json.dumps(doc, allow_nan=False)


def render_joint(snap: NodeSnapshot) -> str | None:
    """The snapshot's window joint histograms as the ``/joint`` document, None when it carries
    none: ``{"buckets": B, "pairs": [[x, y], ..], "gpus": {gpu_id: [{"x": name, "y": name,
    "le_x": [B], "le_y": [B], "counts": [[B + 1] x (B + 1)], "rows": sum}, ..]}}``;
    ``counts[i][j]`` is the number of rows with x in bin i and y in bin j (per bin, the last
    being everything above the last bound), ``rows`` the rows in which both were valid."""
    joint = getattr(snap, "window_joint", None)
    pairs = getattr(snap, "window_joint_pairs", None)
    bounds = getattr(snap, "window_joint_bounds", None)
    if joint is None or pairs is None or bounds is None:
        return None
    joint, bounds = np.asarray(joint), np.asarray(bounds)
    series = list(snap.window_series)
    gpus = {}
    for g, gid in enumerate(snap.gpu_ids):
        gpus[gid] = [{"x": series[a], "y": series[b], "le_x": [float(v) for v in bounds[g, a]],
                      "le_y": [float(v) for v in bounds[g, b]], "counts": joint[g, k].tolist(),
                      "rows": int(joint[g, k].sum())} for k, (a, b) in enumerate(pairs)]
    doc = {"buckets": int(joint.shape[2]) - 1, "pairs": [[series[a], series[b]] for a, b in pairs], "gpus": gpus}
    return json.dumps(doc, allow_nan=False)


def render_autocorr(snap: NodeSnapshot) -> str | None:
    """The snapshot's window autocorrelation as the ``/autocorr`` document, None when it carries
    none: ``{"lags": L, "span": N, "series": [...], "gpus": {gpu_id: {metric: {"acf": [L + 1],
    "pairs": [L + 1], "period_samples", "strength"}}}}``; ``pairs`` is ``n_k``, the pairs of valid
    samples behind each lag; a lag without an acf and a series without a period are null."""
    sums = getattr(snap, "window_autocorr", None)
    if sums is None:
        return None
    from ..ops.window_autocorr import correlogram, pick_period

    sums = np.asarray(sums)
    series = list(snap.window_series)
    gpus = {}
    for g, gid in enumerate(snap.gpu_ids):
        gpus[gid] = {}
        for s, m in enumerate(series):
            acf = correlogram(sums[g, s])
            period, strength = pick_period(acf)
            gpus[gid][m] = {"acf": _nullable(acf), "pairs": [int(v) for v in sums[g, s, :, 0]],
                            "period_samples": period, "strength": strength}
    span = getattr(snap, "window_autocorr_span", None)
    doc = {"lags": int(sums.shape[2]) - 1, "span": int(span) if span is not None else None, "series": series, "gpus": gpus}
    return json.dumps(doc, allow_nan=False)


def render_periods(snap: NodeSnapshot) -> str | None:
    """The snapshot's window period trend as the ``/periods`` document, None when it carries none:
    ``{"columns": P, "lags": L, "span": N, "age_rows": [P + 1], "series": [...], "gpus": {gpu_id:
    {metric: {"period_samples": [P + 1], "strength": [P + 1], "rows": [P + 1]}}}}``; ``rows`` is
    ``n_0``, the valid samples of each slot; a slot without a period and the age of an empty slot
    are null."""
    sums = getattr(snap, "window_periods", None)
    if sums is None:
        return None
    from ..ops.window_periods import slot_periods

    sums = np.asarray(sums)
    series = list(snap.window_series)
    gpus = {}
    for g, gid in enumerate(snap.gpu_ids):
        period, strength, valid = slot_periods(sums[g])
        gpus[gid] = {m: {"period_samples": [None if v != v else int(v) for v in period[s]], "strength": _nullable(strength[s]),
                         "rows": [int(v) for v in valid[s]]} for s, m in enumerate(series)}
    span, age = getattr(snap, "window_periods_span", None), getattr(snap, "window_periods_age_rows", None)
    doc = {"columns": int(sums.shape[2]) - 1, "lags": int(sums.shape[3]) - 1, "span": int(span) if span is not None else None,
           "age_rows": _nullable(age) if age is not None else None, "series": series, "gpus": gpus}
    return json.dumps(doc, allow_nan=False)


def render_xcorr(snap: NodeSnapshot) -> str | None:
    """The snapshot's window cross-correlation as the ``/xcorr`` document, None when it carries
    none: ``{"lags": L, "span": N, "pairs": [[x, y], ..], "gpus": {gpu_id: [{"x", "y", "ccf": [2L + 1],
    "pairs": [2L + 1], "lag_samples", "correlation"}, ..]}}``; ``ccf`` runs over lags ``-L .. L``, the
    inner ``pairs`` is ``n_k``, the pairs of valid samples behind each lag; a lag without a
    coefficient and a pair without a lag are null."""
    sums = getattr(snap, "window_xcorr", None)
    if sums is None:
        return None
    from ..ops.window_xcorr import cross_correlogram, pick_lag

    sums = np.asarray(sums)
    series = list(snap.window_series)
    names = [[series[a], series[b]] for a, b in snap.window_xcorr_pairs]
    gpus = {}
    for g, gid in enumerate(snap.gpu_ids):
        gpus[gid] = []
        for k, (x, y) in enumerate(names):
            ccf = cross_correlogram(sums[g, k])
            lag, r = pick_lag(ccf)
            gpus[gid].append({"x": x, "y": y, "ccf": _nullable(ccf), "pairs": [int(v) for v in sums[g, k, :, 0]],
                              "lag_samples": lag, "correlation": r})
    span = getattr(snap, "window_xcorr_span", None)
    doc = {"lags": int(sums.shape[2]) // 2, "span": int(span) if span is not None else None, "pairs": names, "gpus": gpus}
    return json.dumps(doc, allow_nan=False)


class Exporter:
    """Serves a ``SnapshotSource`` as ``/metrics`` (and ``/trend``, ``/heatmap``, ``/joint``, ``/quantiles``, ``/autocorr``, ``/xcorr``, ``/periods``). With window buckets on,
    ``rocmdash_window_bucket`` / ``rocmdash_node_window_bucket`` carry exact integer counts
    for any window the source keeps: up to 32768 samples from the resident sorted windows,
    longer windows (up to 2^26) streamed from the device rings and printed from float64."""

    def __init__(self, source: SnapshotSource, hostname: str | None = None):
        self.source = source
        self.hostname = hostname or socket.gethostname()
        self.scrapes = 0
        self.errors = 0
        self.last_scrape_s = 0.0
        self.scrape_hist = LatencyHistogram("rocmdash_exporter_scrape_latency_seconds", "Collection time per scrape")
        self._server = None
        self._cached = (None, None, "")  # (snapshot, extra, rendered body) of the last scrape

    def render(self) -> str:
        t0 = time.perf_counter()
        try:
            snap, extra = self.source.collect()
            if snap is self._cached[0] and extra is self._cached[1]:
                body = self._cached[2]  # same refresh as the last scrape (node service: 1 Hz)
            else:
                body = render_snapshot(snap, hostname=self.hostname)
                if extra is not None:
                    body += extra.text()
                self._cached = (snap, extra, body)
        except Exception:
            self.errors += 1
            log.exception("collect failed")
            body = ""
        self.scrapes += 1
        self.last_scrape_s = time.perf_counter() - t0
        self.scrape_hist.observe(self.last_scrape_s)
        own = Exposition()
        self.scrape_hist.add_to(own)
        own.add("rocmdash_exporter_scrapes_total", self.scrapes, {}, "Scrapes served", "counter")
        own.add("rocmdash_exporter_errors_total", self.errors, {}, "Scrapes whose collection failed", "counter")
        own.add("rocmdash_exporter_scrape_seconds", self.last_scrape_s, {}, "Duration of the last collection")
        return body + own.text()

    def trend(self) -> str | None:
        """The ``/trend`` document of a fresh collection; None when the source has no window
        trend (the option is off) or the collection failed."""
        try:
            snap, _ = self.source.collect()
            return render_trend(snap)
        except Exception:
            self.errors += 1
            log.exception("collect failed")
            return None

    def quantiles(self) -> str | None:
        """The ``/quantiles`` document of a fresh collection; None when the source has no window
        quantile trend (the option is off) or the collection failed."""
        try:
            snap, _ = self.source.collect()
            return render_quantiles(snap)
        except Exception:
            self.errors += 1
            log.exception("collect failed")
            return None

    def heatmap(self) -> str | None:
        """The ``/heatmap`` document of a fresh collection; None when the source has no window
        heatmap (the option is off) or the collection failed."""
        try:
            snap, _ = self.source.collect()
            return render_heatmap(snap)
        except Exception:
            self.errors += 1
            log.exception("collect failed")
            return None

    def xcorr(self) -> str | None:
        """The ``/xcorr`` document of a fresh collection; None when the source has no window
        cross-correlation (the option is off) or the collection failed."""
        try:
            snap, _ = self.source.collect()
            return render_xcorr(snap)
        except Exception:
            self.errors += 1
            log.exception("collect failed")
            return None

    def periods(self) -> str | None:
        """The ``/periods`` document of a fresh collection; None when the source has no window
        period trend (the option is off) or the collection failed."""
        try:
            snap, _ = self.source.collect()
            return render_periods(snap)
        except Exception:
            self.errors += 1
            log.exception("collect failed")
            return None

    def autocorr(self) -> str | None:
        """The ``/autocorr`` document of a fresh collection; None when the source has no window
        autocorrelation (the option is off) or the collection failed."""
        try:
            snap, _ = self.source.collect()
            return render_autocorr(snap)
        except Exception:
            self.errors += 1
            log.exception("collect failed")
            return None

    def joint(self) -> str | None:
        """The ``/joint`` document of a fresh collection; None when the source has no window
        joint histogram (the option is off) or the collection failed."""
        try:
            snap, _ = self.source.collect()
            return render_joint(snap)
        except Exception:
            self.errors += 1
            log.exception("collect failed")
            return None

    def health(self) -> tuple:
        """(ok, message) for /healthz: the source's own verdict when it has one (the
        node service reports unhealthy when its refresh loop stalls), else OK."""
        h = getattr(self.source, "health", None)
        if h is None:
            return True, "OK"
        try:
            return h()
        except Exception as e:  # a failing health check is unhealthy, not a 500
            return False, f"health check failed: {e}"

    def serve(self, host: str = "0.0.0.0", port: int = 9400) -> ThreadingHTTPServer:
        exporter = self

        class Handler(BaseHTTPRequestHandler):
            protocol_version = "HTTP/1.1"
            # headers and body leave in two writes: without TCP_NODELAY the body waits for
            # the client's delayed ACK of the headers (~40 ms per keep-alive request)
            disable_nagle_algorithm = True

            def log_message(self, *a):
                pass

            def do_GET(self):
                if self.path.split("?")[0] == "/metrics":
                    body = exporter.render().encode()
                    ctype = CONTENT_TYPE
                    code = 200
                elif self.path.split("?")[0] == "/trend":
                    doc = exporter.trend()
                    if doc is None:
                        body, ctype, code = b"no window trend (start with --window-trend P)\n", "text/plain", 404
                    else:
                        body, ctype, code = doc.encode(), "application/json", 200
                elif self.path.split("?")[0] == "/heatmap":
                    doc = exporter.heatmap()
                    if doc is None:
                        body, ctype, code = b"no window heatmap (start with --window-heatmap PxB)\n", "text/plain", 404
                    else:
                        body, ctype, code = doc.encode(), "application/json", 200
                elif self.path.split("?")[0] == "/xcorr":
                    doc = exporter.xcorr()
                    if doc is None:
                        body, ctype, code = b"no window cross-correlation (start with --window-xcorr PAIRS[/L[/SPAN]])\n", "text/plain", 404
                    else:
                        body, ctype, code = doc.encode(), "application/json", 200
                elif self.path.split("?")[0] == "/periods":
                    doc = exporter.periods()
                    if doc is None:
                        body, ctype, code = b"no window period trend (start with --window-periods P[/L[/SPAN]])\n", "text/plain", 404
                    else:
                        body, ctype, code = doc.encode(), "application/json", 200
                elif self.path.split("?")[0] == "/autocorr":
                    doc = exporter.autocorr()
                    if doc is None:
                        body, ctype, code = b"no window autocorrelation (start with --window-autocorr L[/SPAN])\n", "text/plain", 404
                    else:
                        body, ctype, code = doc.encode(), "application/json", 200
                elif self.path.split("?")[0] == "/joint":
                    doc = exporter.joint()
                    if doc is None:
                        body, ctype, code = b"no window joint histogram (start with --window-joint SPEC)\n", "text/plain", 404
                    else:
                        body, ctype, code = doc.encode(), "application/json", 200
                elif self.path.split("?")[0] == "/quantiles":
                    doc = exporter.quantiles()
                    if doc is None:
                        body, ctype, code = (b"no window quantile trend (start with --window-quantiles P)\n", "text/plain",
                                             404)
                    else:
                        body, ctype, code = doc.encode(), "application/json", 200
                elif self.path in ("/healthz", "/-/healthy"):
                    ok, msg = exporter.health()
                    body, ctype, code = (msg + "\n").encode(), "text/plain", 200 if ok else 503
                else:
                    body, ctype, code = b"not found\n", "text/plain", 404
                self.send_response(code)
                self.send_header("Content-Type", ctype)
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                self.wfile.write(body)

        srv = ThreadingHTTPServer((host, port), Handler)
        srv.daemon_threads = True
        threading.Thread(target=srv.serve_forever, name="rocmdash-exporter", daemon=True).start()
        self._server = srv
        return srv

    @property
    def port(self) -> int:
        return self._server.server_address[1] if self._server else 0

    def close(self) -> None:
        if self._server is not None:
            self._server.shutdown()
            self._server.server_close()
            self._server = None
        self.source.close()


def main(argv=None) -> int:
    from .. import config

    ap = argparse.ArgumentParser(description="rocmdash node exporter (amd_gpu_* + window statistics)")
    ap.add_argument("--host", default="0.0.0.0")
    ap.add_argument("--port", type=int, default=config.EXPORTER_PORT)
    ap.add_argument("--synthetic", type=int, default=0, help="serve a synthetic node with N GPUs")
    ap.add_argument("--source", default="auto", choices=["auto", "hw", "synthetic", "replay"])
    ap.add_argument("--replay", default=None, metavar="NPZ", help="the recording --source replay plays")
    ap.add_argument("--counters", default="auto", choices=["auto", "hw", "synthetic", "off"])
    ap.add_argument("--window-buckets", type=int, default=None, metavar="B",
                    help="also export every series' window as B cumulative le-buckets (1..63; default "
                         "ROCMDASH_WINDOW_BUCKETS, else off)")
    ap.add_argument("--window-trend", type=int, default=None, metavar="P",
                    help="also serve GET /trend: every series' window as P + 1 columns of min / max / mean / count "
                         "(a power of two in 8..1024; default ROCMDASH_WINDOW_TREND, else off)")
    ap.add_argument("--window-excursions", default=None, metavar="F1,F2,..",
                    help="also export every series' episodes above these fractions of its axis: 1 to 4 increasing "
                         "fractions in (0, 1], e.g. 0.5,0.9 (default ROCMDASH_WINDOW_EXCURSIONS, else off)")
    ap.add_argument("--window-heatmap", default=None, metavar="PxB",
                    help="also serve GET /heatmap: every series' window as P + 1 columns of B + 1 bin counts, e.g. "
                         "64x16 (P a power of two in 8..1024, B in 1..63; default ROCMDASH_WINDOW_HEATMAP, else off)")
    ap.add_argument("--window-joint", default=None, metavar="SPEC",
                    help="also serve GET /joint: joint histograms of pairs of series of one ring; SPEC is 'default' or "
                         "comma-separated metricA:metricB (amd_gpu_ optional), 1 to 8 pairs, with an optional /B "
                         "(buckets per axis, 1..31, default 16) (default ROCMDASH_WINDOW_JOINT, else off)")
    ap.add_argument("--window-quantiles", type=int, default=None, metavar="P",
                    help="also serve GET /quantiles: every series' window as P + 1 columns of its exact percentiles "
                         "and their count (a power of two in 8..1024; default ROCMDASH_WINDOW_QUANTILES, else off)")
    ap.add_argument("--window-autocorr", default=None, metavar="L[/SPAN]",
                    help="also serve GET /autocorr and the rocmdash_window_period_* gauges: every series' autocorrelation at "
                         "lags 0..L (1..1024; 255, 511 and 1023 fill the kernel's blocks of 256 lags) over the newest SPAN rows of its window (a power of two in 64..1048576, "
                         "default 65536) and its period (default ROCMDASH_WINDOW_AUTOCORR, else off)")
    ap.add_argument("--window-xcorr", default=None, metavar="PAIRS[/L[/SPAN]]",
                    help="also serve GET /xcorr and the rocmdash_window_lag_* gauges: the cross-correlation of pairs of series "
                         "of one ring ('default' or metricA:metricB,.., as --window-joint) at lags -L..L (1..1024, default 255) "
                         "over the newest SPAN rows of their window (a power of two in 64..1048576, default 65536) and the "
                         "lag of each pair (default ROCMDASH_WINDOW_XCORR, else off)")
    ap.add_argument("--window-periods", default=None, metavar="P[/L[/SPAN]]",
                    help="also serve GET /periods: every series' period per trend column - the autocorrelation at lags 0..L "
                         "(default 255; at most half a column) of each of P + 1 columns (a power of two in 8..64) of the "
                         "newest SPAN rows of its window (a power of two in 512..1048576, default min(window, 65536)) "
                         "(default ROCMDASH_WINDOW_PERIODS, else off)")
    args = ap.parse_args(argv)
    if args.window_periods is not None:
        from ..ops.window_periods import parse_periods

        try:
            parse_periods(args.window_periods, config.SamplerConfig().window)
        except ValueError as e:
            ap.error(f"--window-periods: {e}")
    if args.window_xcorr is not None:
        from ..models.schema import CTR_FIELDS, SMI_FIELDS
        from ..ops.window_xcorr import parse_xcorr

        try:
            parse_xcorr(args.window_xcorr, SMI_FIELDS + CTR_FIELDS, (len(SMI_FIELDS), len(CTR_FIELDS)))
        except ValueError as e:
            ap.error(f"--window-xcorr: {e}")
    if args.window_autocorr is not None:
        from ..ops.window_autocorr import parse_autocorr

        try:
            parse_autocorr(args.window_autocorr)
        except ValueError as e:
            ap.error(f"--window-autocorr: {e}")
    if args.window_joint is not None:
        from ..models.schema import CTR_FIELDS, SMI_FIELDS
        from ..ops.window_joint import parse_joint

        try:
            parse_joint(args.window_joint, SMI_FIELDS + CTR_FIELDS, (len(SMI_FIELDS), len(CTR_FIELDS)))
        except ValueError as e:
            ap.error(f"--window-joint: {e}")
    if args.window_heatmap is not None:
        from ..ops.window_heatmap import parse_heatmap

        try:
            parse_heatmap(args.window_heatmap)
        except ValueError as e:
            ap.error(f"--window-heatmap: {e}")
    if args.window_excursions is not None:
        from ..ops.window_excursions import parse_fractions

        try:
            parse_fractions(args.window_excursions)
        except ValueError as e:
            ap.error(f"--window-excursions: {e}")
    logging.basicConfig(level=logging.INFO)
    src = SyntheticSource(args.synthetic) if args.synthetic else LocalNodeSource(
        source=args.source, counters=args.counters, window_buckets=args.window_buckets, window_trend=args.window_trend,
        window_excursions=args.window_excursions, replay=args.replay, window_heatmap=args.window_heatmap,
        window_joint=args.window_joint, window_quantiles=args.window_quantiles,
        window_autocorr=args.window_autocorr, window_xcorr=args.window_xcorr, window_periods=args.window_periods)
    exp = Exporter(src)
    exp.serve(args.host, args.port)
    log.info("serving /metrics on %s:%d", args.host, exp.port)
    try:
        while True:
            time.sleep(3600)
    except KeyboardInterrupt:
        exp.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
