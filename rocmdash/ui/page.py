"""The Streamlit page: same layout, strings, widget keys and behaviour as the reference.

Reference: ``app.py:247-486`` (``main``), ``app.py:234-245`` (``create_visualization``).
Layout, in order: title + caption; "Display Settings" with the gauge toggle; "GPU
Selection" as a 4-column checkbox grid (keys ``gpu_checkbox_<id>``, first GPU selected
by default, stale selections dropped); debug sidebar; then a placeholder that is
redrawn every ``REFRESH_INTERVAL`` seconds with the average row, one row per
selected GPU, the statistics table and the "Last updated" footer.

Data sources (``ROCMDASH_DATA_SOURCE``):
  * ``prometheus`` (default): the reference's two PromQL queries against
    ``PROMETHEUS_METRICS_ENDPOINT`` (rocmdash.prom.query);
  * ``native``: one scrape per refresh of the local rank-per-GPU node service
    (``rocmdash.serve``, ``ROCMDASH_NODE_ENDPOINT``, default
    ``http://127.0.0.1:9400/metrics``): the RCCL-gathered node tensor - every series,
    window and node-window statistics, per-XCD detail - with no Prometheus between;
  * ``synthetic``: a synthetic 8-GPU node (demo / CPU).

The frame (figures, averages, tables) is built by ``rocmdash.viz.panels.build_frame``;
this module only maps it onto Streamlit calls.
"""

from __future__ import annotations

import os
import time
from datetime import datetime

from .. import config
from ..models.gpu_models import GPU_NAME_RESOLVE, GPU_POWER_LIMITS
from ..prom import query as _query
from ..viz.figures import (  # noqa: F401
    GAUGE_COLORS,
    create_gauge,
    create_horizontal_bar,
    figure_from_spec,
    get_color_for_value,
)
from ..viz.panels import NodeSnapshot, build_frame, natural_key, power_axis_max

PAGE_CONFIG = dict(
    page_title="GPU Metrics Dashboard",
    page_icon="📊",
    layout="wide",
    initial_sidebar_state="collapsed",
)


def _st():
    import streamlit as st

    return st


def get_power_limit(card_model):
    """``app.py:229-232`` (dead code in the reference, kept for API compatibility)."""
    resolved_model = GPU_NAME_RESOLVE.get(card_model, card_model)
    return GPU_POWER_LIMITS.get(resolved_model, GPU_POWER_LIMITS["default"])


def create_visualization(value, title, max_val, height, key, gpu_id=None, gpu_metrics_df=None):
    """Style dispatch (``app.py:234-245``): power panels use the GPU's power limit as
    the axis max; gauge or bar per ``st.session_state.use_gauge``. ``key`` is unused,
    as in the reference. ``gpu_metrics_df`` may be a DataFrame or a NodeSnapshot."""
    if title.endswith("Power Usage (W)") and gpu_id is not None and gpu_metrics_df is not None:
        if isinstance(gpu_metrics_df, NodeSnapshot):
            max_val = gpu_metrics_df.power_max(gpu_id)
        else:
            max_val = power_axis_max(gpu_metrics_df.loc[gpu_id, "card_model"])
    use_gauge = True
    try:
        use_gauge = bool(_st().session_state.use_gauge)
    except Exception:
        pass
    if use_gauge:
        return create_gauge(value, title, max_val=max_val, height=height)
    return create_horizontal_bar(value, title, max_val=max_val, height=height)


def fetch_gpu_metrics():
    """``app.py:153-227`` contract: ``(df, stats)`` or ``(None, None)`` + error banner."""
    return _query.fetch_gpu_metrics(on_error=lambda m: _st().error(m))


# ------------------------------------------------------------------ data sources
class _DataSource:
    _synthetic = None

    def __init__(self, kind: str | None = None):
        self.kind = (kind or os.environ.get("ROCMDASH_DATA_SOURCE", "prometheus")).lower()
        self.client = _query.PrometheusClient() if self.kind == "prometheus" else None

    def snapshot(self) -> NodeSnapshot:
        if self.kind == "prometheus":
            return _query.fetch_node_snapshot(self.client)
        if self.kind == "synthetic":
            from ..prom.exporter import SyntheticSource

            if _DataSource._synthetic is None:
                _DataSource._synthetic = SyntheticSource(int(os.environ.get("ROCMDASH_SYNTHETIC_GPUS", "8")))
            return _DataSource._synthetic.collect()[0]
        if self.kind == "native":
            return _query.fetch_service_snapshot()
        raise ValueError(f"unknown ROCMDASH_DATA_SOURCE {self.kind!r}")

    def fetch(self):
        """(snapshot | None); errors go to the banner like app.py:226."""
        try:
            return self.snapshot()
        except Exception as e:
            _st().error(f"Error fetching GPU metrics: {str(e)}")
            return None


def node_window_table(snap: NodeSnapshot) -> dict | None:
    """{series: {stat: value}} of the node-wide window statistics (None if absent)."""
    if snap.node_window is None:
        return None
    from ..models.schema import STAT_NAMES

    return {series: {k: round(float(snap.node_window[i, j]), 2) for j, k in enumerate(STAT_NAMES) if k != "last"}
            for i, series in enumerate(snap.window_series)}


BUCKET_SHARES = (50, 75, 90)  # % of a series' axis (its highest finite bound)


def window_bucket_table(snap: NodeSnapshot) -> dict | None:
    """{series: {"> 50% of axis": share, ...}}: the share (%) of the node's window - every
    GPU's last W samples - above 50 / 75 / 90 % of each series' axis, from the node's
    le-buckets (``rocmdash.ops.window_buckets.share_above``; None if absent)."""
    node = getattr(snap, "node_window_buckets", None)
    bounds = getattr(snap, "window_bucket_bounds", None)
    if node is None or bounds is None:
        return None
    from ..ops.window_buckets import share_above

    table = {}
    for i, series in enumerate(snap.window_series):
        row = {"axis": float(bounds[i][-1]), "samples": int(node[i][-1])}
        for pct in BUCKET_SHARES:
            share = share_above(node[i], bounds[i], float(bounds[i][-1]) * pct / 100.0)
            row[f"> {pct}% of axis (%)"] = round(100.0 * share, 2)
        table[series] = row
    return table


def window_trend_figures(snap: NodeSnapshot, selected=None, height: int = 220) -> list | None:
    """[(key, Figure)]: per selected GPU the window trend (``rocmdash.ops.window_trend``) of
    every panel metric the snapshot's trend has - utilisation, temperature, power and the
    extended panels - as a min..max band and a mean line over seconds (None if the snapshot
    carries no trend). The slots' ages are rows of the first ring; a series' seconds are
    those rows times its own source's period (amd-smi or device counters)."""
    trend = getattr(snap, "window_trend", None)
    age = getattr(snap, "window_trend_age_rows", None)
    if trend is None or age is None:
        return None
    from ..models.schema import CTR_FIELDS
    from ..viz.figures import create_trend
    from ..viz.panels import EXTENDED_PANELS, POWER, TEMP, UTIL

    cfg = config.SamplerConfig()
    index = {s: i for i, s in enumerate(snap.window_series)}
    sel = set(str(g) for g in selected) if selected is not None else None
    figs = []
    for g, gid in enumerate(snap.gpu_ids):
        if sel is not None and gid not in sel:
            continue
        panels = [(UTIL, "GPU Utilization (%)", "gpu_util", 100.0), (TEMP, "Temperature (°C)", "temp", 100.0),
                  (POWER, "Power Usage (W)", "power", snap.power_max(gid))] + list(EXTENDED_PANELS)
        for col, title, key, mx in panels:
            s = index.get(col)
            if s is None:
                continue
            period = 1.0 / (cfg.counter_hz if col in CTR_FIELDS else cfg.smi_hz)
            t = trend[g, s]
            figs.append((f"plot_trend_{key}_{gid}_", create_trend(f"GPU {gid}: {title}", [a * period for a in age],
                                                                   t[:, 0], t[:, 1], t[:, 2], mx, height)))
    return figs


def window_quantile_figures(snap: NodeSnapshot, selected=None, height: int = 220) -> list | None:
    """[(key, Figure)]: per selected GPU the window quantile trend
    (``rocmdash.ops.window_quantiles``) of every panel metric the snapshot's has - the metrics
    and the seconds of ``window_trend_figures`` - as three percentile lines over time (None if
    the snapshot carries none)."""
    quant = getattr(snap, "window_quantiles", None)
    age = getattr(snap, "window_quantiles_age_rows", None)
    pct = getattr(snap, "window_quantiles_pct", None)
    if quant is None or age is None or pct is None:
        return None
    from ..models.schema import CTR_FIELDS
    from ..viz.figures import create_quantiles
    from ..viz.panels import EXTENDED_PANELS, POWER, TEMP, UTIL

    cfg = config.SamplerConfig()
    index = {s: i for i, s in enumerate(snap.window_series)}
    sel = set(str(g) for g in selected) if selected is not None else None
    figs = []
    for g, gid in enumerate(snap.gpu_ids):
        if sel is not None and gid not in sel:
            continue
        panels = [(UTIL, "GPU Utilization (%)", "gpu_util", 100.0), (TEMP, "Temperature (°C)", "temp", 100.0),
                  (POWER, "Power Usage (W)", "power", snap.power_max(gid))] + list(EXTENDED_PANELS)
        for col, title, key, mx in panels:
            s = index.get(col)
            if s is None:
                continue
            period = 1.0 / (cfg.counter_hz if col in CTR_FIELDS else cfg.smi_hz)
            q = quant[g, s]
            figs.append((f"plot_quantiles_{key}_{gid}_",
                         create_quantiles(f"GPU {gid}: {title}", [a * period for a in age], pct,
                                          (q[:, 0], q[:, 1], q[:, 2]), mx, height)))
    return figs


def window_autocorr_figures(snap: NodeSnapshot, selected=None, height: int = 220) -> list | None:
    """[(key, Figure)]: per selected GPU the correlogram (``rocmdash.ops.window_autocorr``) of
    every panel metric the snapshot's autocorrelation has - the metrics of
    ``window_trend_figures`` - as a line over the lag with a marker at the period (None if the
    snapshot carries none)."""
    sums = getattr(snap, "window_autocorr", None)
    if sums is None:
        return None
    from ..ops.window_autocorr import correlogram, pick_period
    from ..viz.figures import create_autocorr
    from ..viz.panels import EXTENDED_PANELS, POWER, TEMP, UTIL

    index = {s: i for i, s in enumerate(snap.window_series)}
    sel = set(str(g) for g in selected) if selected is not None else None
    figs = []
    for g, gid in enumerate(snap.gpu_ids):
        if sel is not None and gid not in sel:
            continue
        panels = [(UTIL, "GPU Utilization (%)", "gpu_util", 100.0), (TEMP, "Temperature (°C)", "temp", 100.0),
                  (POWER, "Power Usage (W)", "power", snap.power_max(gid))] + list(EXTENDED_PANELS)
        for col, title, key, _ in panels:
            s = index.get(col)
            if s is None:
                continue
            acf = correlogram(sums[g][s])
            period, _ = pick_period(acf)
            figs.append((f"plot_autocorr_{key}_{gid}_",
                         create_autocorr(f"GPU {gid}: {title}", acf, [title], [period], height)))
    return figs


def window_periods_figures(snap: NodeSnapshot, selected=None, height: int = 220) -> list | None:
    """[(key, Figure)]: per selected GPU the window period trend (``rocmdash.ops.window_periods``)
    of every panel metric the snapshot's has - the metrics and the seconds of
    ``window_trend_figures`` - as the period of each slot over time (None if the snapshot carries
    none)."""
    sums = getattr(snap, "window_periods", None)
    age = getattr(snap, "window_periods_age_rows", None)
    if sums is None or age is None:
        return None
    from ..models.schema import CTR_FIELDS
    from ..ops.window_periods import slot_periods
    from ..viz.figures import create_periods
    from ..viz.panels import EXTENDED_PANELS, POWER, TEMP, UTIL

    cfg = config.SamplerConfig()
    index = {s: i for i, s in enumerate(snap.window_series)}
    sel = set(str(g) for g in selected) if selected is not None else None
    figs = []
    for g, gid in enumerate(snap.gpu_ids):
        if sel is not None and gid not in sel:
            continue
        panels = [(UTIL, "GPU Utilization (%)", "gpu_util", 100.0), (TEMP, "Temperature (°C)", "temp", 100.0),
                  (POWER, "Power Usage (W)", "power", snap.power_max(gid))] + list(EXTENDED_PANELS)
        for col, title, key, _ in panels:
            s = index.get(col)
            if s is None:
                continue
            seconds = 1.0 / (cfg.counter_hz if col in CTR_FIELDS else cfg.smi_hz)
            period, strength, _ = slot_periods(sums[g][s : s + 1])
            figs.append((f"plot_periods_{key}_{gid}_",
                         create_periods(f"GPU {gid}: {title}", [a * seconds for a in age], period[0], strength[0], height)))
    return figs


def window_xcorr_figures(snap: NodeSnapshot, selected=None, height: int = 220) -> list | None:
    """[(key, Figure)]: per selected GPU and pair the cross-correlogram
    (``rocmdash.ops.window_xcorr``) the snapshot carries, as a line over the lag ``-L .. L`` with a
    zero line and a marker at the pair's lag (None if the snapshot carries none)."""
    sums = getattr(snap, "window_xcorr", None)
    pairs = getattr(snap, "window_xcorr_pairs", None)
    if sums is None or pairs is None:
        return None
    from ..ops.window_xcorr import cross_correlogram, pick_lag
    from ..viz.figures import create_xcorr

    series = list(snap.window_series)
    short = lambda m: m[len("amd_gpu_"):] if m.startswith("amd_gpu_") else m  # noqa: E731
    sel = set(str(g) for g in selected) if selected is not None else None
    figs = []
    for g, gid in enumerate(snap.gpu_ids):
        if sel is not None and gid not in sel:
            continue
        for k, (a, b) in enumerate(pairs):
            x, y = short(series[a]), short(series[b])
            ccf = cross_correlogram(sums[g][k])
            lag, _ = pick_lag(ccf)
            figs.append((f"plot_xcorr_{x}_{y}_{gid}_", create_xcorr(f"GPU {gid}: {y} after {x}", ccf, lag, x, y, height)))
    return figs


def window_heatmap_figures(snap: NodeSnapshot, selected=None, height: int = 220) -> list | None:
    """[(key, Figure)]: per selected GPU the window heatmap (``rocmdash.ops.window_heatmap``)
    of every panel metric the snapshot's heatmap has - the metrics and the seconds of
    ``window_trend_figures`` - as counts per bin over time (None if the snapshot carries no
    heatmap)."""
    heat = getattr(snap, "window_heatmap", None)
    bounds = getattr(snap, "window_heatmap_bounds", None)
    age = getattr(snap, "window_heatmap_age_rows", None)
    if heat is None or bounds is None or age is None:
        return None
    from ..models.schema import CTR_FIELDS
    from ..viz.figures import create_heatmap
    from ..viz.panels import EXTENDED_PANELS, POWER, TEMP, UTIL

    cfg = config.SamplerConfig()
    index = {s: i for i, s in enumerate(snap.window_series)}
    sel = set(str(g) for g in selected) if selected is not None else None
    figs = []
    for g, gid in enumerate(snap.gpu_ids):
        if sel is not None and gid not in sel:
            continue
        panels = [(UTIL, "GPU Utilization (%)", "gpu_util"), (TEMP, "Temperature (°C)", "temp"),
                  (POWER, "Power Usage (W)", "power")] + [p[:3] for p in EXTENDED_PANELS]
        for col, title, key in panels:
            s = index.get(col)
            if s is None:
                continue
            period = 1.0 / (cfg.counter_hz if col in CTR_FIELDS else cfg.smi_hz)
            figs.append((f"plot_heatmap_{key}_{gid}_", create_heatmap(f"GPU {gid}: {title}", [a * period for a in age],
                                                                       bounds[g][s], heat[g, s], height)))
    return figs


def window_joint_figures(snap: NodeSnapshot, selected=None, height: int = 260) -> list | None:
    """[(key, Figure)]: per selected GPU and pair the window joint histogram
    (``rocmdash.ops.window_joint``) the snapshot carries - the first series on x, the second on
    y, rows as colour (None if the snapshot carries none)."""
    joint = getattr(snap, "window_joint", None)
    pairs = getattr(snap, "window_joint_pairs", None)
    bounds = getattr(snap, "window_joint_bounds", None)
    if joint is None or pairs is None or bounds is None:
        return None
    from ..viz.figures import create_joint

    series = list(snap.window_series)
    short = lambda m: m[len("amd_gpu_"):] if m.startswith("amd_gpu_") else m  # noqa: E731
    sel = set(str(g) for g in selected) if selected is not None else None
    figs = []
    for g, gid in enumerate(snap.gpu_ids):
        if sel is not None and gid not in sel:
            continue
        for k, (a, b) in enumerate(pairs):
            x, y = short(series[a]), short(series[b])
            figs.append((f"plot_joint_{x}_{y}_{gid}_", create_joint(f"GPU {gid}: {y} vs {x}", bounds[g][a], bounds[g][b],
                                                                     joint[g][k], x, y, height)))
    return figs


def window_excursion_tables(snap: NodeSnapshot, selected=None) -> dict | None:
    """{"GPU <id>": [{metric, threshold, episodes, longest, current, since}, ...]}: per selected
    GPU one table of the window excursions (``rocmdash.ops.window_excursions``; lengths in
    valid samples), one row per series and threshold (None if the snapshot carries none)."""
    exc = getattr(snap, "window_excursions", None)
    thr = getattr(snap, "window_excursion_thresholds", None)
    if exc is None or thr is None:
        return None
    from ..ops.window_excursions import E_CURRENT, E_EPISODES, E_LONGEST, E_SINCE

    sel = set(str(g) for g in selected) if selected is not None else None
    tables = {}
    for g, gid in enumerate(snap.gpu_ids):
        if sel is not None and gid not in sel:
            continue
        tables[f"GPU {gid}"] = [
            {"metric": series, "threshold": float(thr[si][k]), "episodes": int(exc[g, si, k, E_EPISODES]),
             "longest": int(exc[g, si, k, E_LONGEST]), "current": int(exc[g, si, k, E_CURRENT]),
             "since": int(exc[g, si, k, E_SINCE])}
            for si, series in enumerate(snap.window_series) for k in range(len(thr[si]))]
    return tables or None


def xcd_table(snap: NodeSnapshot, selected=None) -> dict | None:
    """{"GPU <id>": {"XCD <x> busy %": v, "XCD <x> MHz": v, ...}} of the selected GPUs'
    per-XCD detail (None if the data source has none)."""
    xcd = getattr(snap, "xcd", None)
    if xcd is None:
        return None
    sel = set(selected) if selected is not None else None
    table = {}
    for g, gid in enumerate(snap.gpu_ids):
        if sel is not None and gid not in sel:
            continue
        row = {}
        for x in range(xcd.shape[2]):
            if xcd[g, 0, x] != xcd[g, 0, x] and xcd[g, 1, x] != xcd[g, 1, x]:  # NaN: no such XCD
                continue
            row[f"XCD {x} busy %"] = float(xcd[g, 0, x])
            row[f"XCD {x} MHz"] = float(xcd[g, 1, x])
        if row:
            table[f"GPU {gid}"] = row
    return table or None


def _render_frame(st, frame, extended: bool, node_window: dict | None = None, xcd: dict | None = None,
                  buckets: dict | None = None, trend: list | None = None, excursions: dict | None = None,
                  heatmap: list | None = None, joint: list | None = None, quantiles: list | None = None,
                  autocorr: list | None = None, xcorr: list | None = None, periods: list | None = None) -> None:
    st.subheader("Average Metrics (Selected GPUs)")
    avg_cols = st.columns(4)
    for col, (key, spec) in zip(avg_cols, frame.avg_panels):
        with col:
            st.plotly_chart(figure_from_spec(spec).to_dict(), use_container_width=True, key=key)
    st.subheader("Individual GPU Metrics")
    for _, header, panels in frame.gpu_sections:
        st.markdown(header)
        ncols = 4
        for i in range(0, len(panels), ncols):
            cols = st.columns(ncols)
            for col, (key, spec) in zip(cols, panels[i : i + ncols]):
                with col:
                    st.plotly_chart(figure_from_spec(spec).to_dict(), use_container_width=True, key=key)
    st.subheader("GPU Metrics Statistics")
    import pandas as pd

    st.dataframe(pd.DataFrame(frame.stats_table), use_container_width=True)
    if extended and frame.window_table:
        st.subheader("Windowed Statistics (HIP window-stats kernel)")
        rows = {
            (gid, series): stats for gid, per in frame.window_table.items() for series, stats in per.items()
        }
        st.dataframe(pd.DataFrame.from_dict(rows, orient="index"), use_container_width=True)
    if extended and node_window is not None:
        st.subheader("Node-wide Windowed Statistics (all GPUs)")
        st.dataframe(pd.DataFrame(node_window), use_container_width=True)
    if extended and buckets is not None:
        st.subheader("Node-wide Window Distribution (share of samples above 50 / 75 / 90 % of the axis)")
        st.dataframe(pd.DataFrame.from_dict(buckets, orient="index"), use_container_width=True)
    if extended and trend:
        st.subheader("Window Trend (min / max band and mean per column of the window)")
        for i in range(0, len(trend), 4):
            for col, (key, fig) in zip(st.columns(4), trend[i : i + 4]):
                with col:
                    st.plotly_chart(fig.to_dict(), use_container_width=True, key=key)
    if extended and quantiles:
        st.subheader("Window Quantile Trend (exact percentiles per column of the window)")
        for i in range(0, len(quantiles), 4):
            for col, (key, fig) in zip(st.columns(4), quantiles[i : i + 4]):
                with col:
                    st.plotly_chart(fig.to_dict(), use_container_width=True, key=key)
    if extended and autocorr:
        st.subheader("Window Autocorrelation (acf over the lag in samples; the marker is the period)")
        for i in range(0, len(autocorr), 4):
            for col, (key, fig) in zip(st.columns(4), autocorr[i : i + 4]):
                with col:
                    st.plotly_chart(fig.to_dict(), use_container_width=True, key=key)
    if extended and periods:
        st.subheader("Window Period Trend (each column's period in samples; fainter markers are weaker periods)")
        for i in range(0, len(periods), 4):
            for col, (key, fig) in zip(st.columns(4), periods[i : i + 4]):
                with col:
                    st.plotly_chart(fig.to_dict(), use_container_width=True, key=key)
    if extended and xcorr:
        st.subheader("Window Cross-correlation (r over the lag in samples; right of zero the second series follows)")
        for i in range(0, len(xcorr), 4):
            for col, (key, fig) in zip(st.columns(4), xcorr[i : i + 4]):
                with col:
                    st.plotly_chart(fig.to_dict(), use_container_width=True, key=key)
    if extended and heatmap:
        st.subheader("Window Heatmap (samples per bucket and column of the window)")
        for i in range(0, len(heatmap), 4):
            for col, (key, fig) in zip(st.columns(4), heatmap[i : i + 4]):
                with col:
                    st.plotly_chart(fig.to_dict(), use_container_width=True, key=key)
    if extended and joint:
        st.subheader("Window Joint Histograms (rows per pair of buckets of two series)")
        for i in range(0, len(joint), 4):
            for col, (key, fig) in zip(st.columns(4), joint[i : i + 4]):
                with col:
                    st.plotly_chart(fig.to_dict(), use_container_width=True, key=key)
    if extended and excursions:
        st.subheader("Window Excursions (episodes above a threshold; lengths in valid samples)")
        for title, rows in excursions.items():
            st.markdown(f"**{title}**")
            st.dataframe(pd.DataFrame(rows), use_container_width=True)
    if extended and xcd is not None:
        st.subheader("Per-XCD Activity and Clocks")
        st.dataframe(pd.DataFrame.from_dict(xcd, orient="index"), use_container_width=True)
    st.text(frame.updated_text)


def main(max_refreshes: int | None = None, data_source: str | None = None) -> None:
    """The page. ``max_refreshes`` (or ``ROCMDASH_MAX_REFRESHES``) bounds the refresh
    loop for tests; the reference loops forever (``app.py:326``)."""
    st = _st()
    if max_refreshes is None and os.environ.get("ROCMDASH_MAX_REFRESHES"):
        max_refreshes = int(os.environ["ROCMDASH_MAX_REFRESHES"])
    extended = os.environ.get("ROCMDASH_EXTENDED", "0") not in ("0", "", "false")
    st.title("GPU Metrics Dashboard")
    st.markdown("Real-time monitoring of GPU metrics")

    if "selected_gpus" not in st.session_state:
        st.session_state.selected_gpus = []
    if "use_gauge" not in st.session_state:
        st.session_state.use_gauge = True

    st.header("Display Settings")
    use_gauge = st.toggle("Use Gauge Visualization", value=st.session_state.use_gauge)
    st.session_state.use_gauge = use_gauge

    source = _DataSource(data_source)
    snap = source.fetch()
    available_gpus = list(snap.gpu_ids) if snap is not None else []

    st.header("GPU Selection")
    num_columns = 4
    gpu_cols = st.columns(num_columns)
    if "last_selection" not in st.session_state:
        st.session_state.last_selection = None

    sorted_gpus = sorted(available_gpus, key=natural_key)
    st.session_state.selected_gpus = [g for g in st.session_state.selected_gpus if g in sorted_gpus]
    if not st.session_state.selected_gpus and sorted_gpus:
        st.session_state.selected_gpus = [sorted_gpus[0]]

    for i, gpu_id in enumerate(sorted_gpus):
        with gpu_cols[i % num_columns]:
            is_currently_selected = gpu_id in st.session_state.selected_gpus
            is_selected = st.checkbox(f"GPU {gpu_id}", value=is_currently_selected, key=f"gpu_checkbox_{gpu_id}")
            if is_selected != is_currently_selected:
                if is_selected:
                    st.session_state.selected_gpus.append(gpu_id)
                else:
                    st.session_state.selected_gpus.remove(gpu_id)
                st.session_state.last_selection = gpu_id

    st.session_state.selected_gpus.sort(key=natural_key)

    st.sidebar.write("Debug Info:")
    st.sidebar.write("Current selections:", st.session_state.selected_gpus)
    st.sidebar.write("Last selection:", st.session_state.last_selection)

    placeholder = st.empty()
    n = 0
    while max_refreshes is None or n < max_refreshes:
        now = datetime.now()
        with placeholder.container():
            snap = source.fetch()
            if snap is not None:
                frame = build_frame(
                    snap, st.session_state.selected_gpus, use_gauge=st.session_state.use_gauge, extended=extended, now=now
                )
                _render_frame(st, frame, extended, node_window_table(snap) if extended else None,
                              xcd_table(snap, st.session_state.selected_gpus) if extended else None,
                              window_bucket_table(snap) if extended else None,
                              window_trend_figures(snap, st.session_state.selected_gpus) if extended else None,
                              window_excursion_tables(snap, st.session_state.selected_gpus) if extended else None,
                              window_heatmap_figures(snap, st.session_state.selected_gpus) if extended else None,
                              window_joint_figures(snap, st.session_state.selected_gpus) if extended else None,
                              window_quantile_figures(snap, st.session_state.selected_gpus) if extended else None,
                              window_autocorr_figures(snap, st.session_state.selected_gpus) if extended else None,
                              window_xcorr_figures(snap, st.session_state.selected_gpus) if extended else None,
                              window_periods_figures(snap, st.session_state.selected_gpus) if extended else None)
        n += 1
        if max_refreshes is not None and n >= max_refreshes:
            break
        time.sleep(config.REFRESH_INTERVAL)
