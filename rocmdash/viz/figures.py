"""Gauge / bar figure factories that emit Plotly-compatible figure JSON without Plotly.

Reference: ``create_gauge`` (``app.py:70-103``), ``create_horizontal_bar``
(``app.py:105-151``) and ``get_color_for_value`` (``app.py:56-68``). The reference
builds a validated ``plotly.graph_objects.Figure`` per chart and Streamlit then
serialises it; at 8 GPUs that is 36 figures and ~150 ms per refresh on a CPU
(BASELINE.md), i.e. the whole dashboard refresh is Plotly object construction.

Here a figure is a plain ``{"data": [...], "layout": {...}}`` tree built from dict
literals (no validation pass: the trees are fixed by construction and the test suite
checks them against Plotly's own JSON, ``tests/test_viz.py``). The default Plotly
template (~7 KB of JSON, identical for every figure) is serialised ONCE per process
and spliced into each figure's JSON, so a refresh costs a few microseconds per chart.
``Figure.to_plotly()`` gives a real ``go.Figure`` when a consumer needs one.
"""

from __future__ import annotations

import json
import math
from functools import lru_cache

# Colour scheme, verbatim from app.py:41-54.
GAUGE_COLORS = {
    "green": "#2ecc71",  # 0-20% (value bar)
    "light_green": "#27ae60",  # 20-40% (value bar)
    "yellow": "#f1c40f",  # 40-60% (value bar)
    "orange": "#e67e22",  # 60-80% (value bar)
    "red": "#e74c3c",  # 80-100% (value bar)
    # Less saturated colours for gauge plates
    "plate_green": "#a8e6cf",
    "plate_light_green": "#88d8b0",
    "plate_yellow": "#ffd3b6",
    "plate_orange": "#ffaaa5",
    "plate_red": "#ff8b94",
}

_PLATES = ("plate_green", "plate_light_green", "plate_yellow", "plate_orange", "plate_red")


def get_color_for_value(value, max_val):
    """Bar colour by percentage of ``max_val`` (app.py:56-68).

    Same semantics as the reference: inclusive upper bounds at 20/40/60/80 %,
    ``max_val == 0`` raises ``ZeroDivisionError``, NaN falls through to red.
    """
    percentage = (value / max_val) * 100
    if percentage <= 20:
        return GAUGE_COLORS["green"]
    elif percentage <= 40:
        return GAUGE_COLORS["light_green"]
    elif percentage <= 60:
        return GAUGE_COLORS["yellow"]
    elif percentage <= 80:
        return GAUGE_COLORS["orange"]
    return GAUGE_COLORS["red"]


# ----------------------------------------------------------------------------- JSON
def _num(x):
    """Plotly's JSON encoder semantics for a scalar: numpy scalars -> Python numbers,
    NaN / inf -> null; ints stay ints."""
    if x is None:
        return None
    if isinstance(x, bool):
        return x
    if isinstance(x, int):
        return x
    try:
        f = float(x)
    except (TypeError, ValueError):
        return x
    if math.isnan(f) or math.isinf(f):
        return None
    if hasattr(x, "dtype") and getattr(x.dtype, "kind", "f") in "iu":
        return int(x)
    return f


@lru_cache(maxsize=1)
def template_json() -> str:
    """The default Plotly template as JSON (what ``go.Figure().to_json()`` embeds).

    Taken from the installed Plotly when present; without Plotly the layout carries an
    empty template (Plotly.js then uses its own defaults)."""
    try:
        import plotly.io as pio

        name = pio.templates.default
        if not name or name == "none":
            return "{}"
        return json.dumps(pio.templates[name].to_plotly_json(), separators=(",", ":"))
    except Exception:
        return "{}"


def _dumps(obj) -> str:
    return json.dumps(obj, separators=(",", ":"), allow_nan=False)


def _set_path(d: dict, key: str, value) -> None:
    """Plotly 'magic underscore' keys: line_width -> {'line': {'width': ...}}."""
    parts = key.split("_") if key not in _NO_SPLIT else [key]
    cur = d
    for p in parts[:-1]:
        nxt = cur.get(p)
        if not isinstance(nxt, dict):
            nxt = {}
            cur[p] = nxt
        cur = nxt
    cur[parts[-1]] = value


# property names that contain underscores and must not be split
_NO_SPLIT = frozenset({"use_container_width"})


def _merge(dst: dict, src: dict) -> None:
    for k, v in src.items():
        if "_" in k and k not in dst and k not in _NO_SPLIT and k.split("_")[0] in _MAGIC_ROOTS:
            _set_path(dst, k, _clean(v))
        elif isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = _clean(v)


_MAGIC_ROOTS = frozenset({"line", "marker", "title", "xaxis", "yaxis", "font", "legend", "margin"})


def _clean(v):
    if isinstance(v, dict):
        return {k: _clean(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_clean(x) for x in v]
    if isinstance(v, str):
        return v
    return _num(v)


class Figure:
    """Minimal Plotly-figure stand-in: ``data``/``layout`` trees plus the methods the
    reference's factories call (``update_layout``, ``add_shape``) and serialisation.

    ``to_json()`` / ``to_dict()`` are structurally identical to Plotly's for the
    figures this module builds (checked in tests/test_viz.py).

    Figures made by the factories below are *lazy*: they keep (kind, value, title,
    axis range, height) and serialise through a cached JSON template of that panel
    (only the value and the band colour change between refreshes), so a gauge costs a
    few string concatenations per refresh. The ``data`` / ``layout`` trees are built
    only when accessed; any mutation switches the figure to the tree path.
    """

    __slots__ = ("_data", "_layout", "_fast")

    def __init__(self, data=None, layout=None, _fast=None):
        self._fast = _fast
        if _fast is None:
            self._data = list(data or [])
            self._layout = dict(layout or {})
        else:
            self._data = None
            self._layout = None

    def _materialize(self):
        if self._data is None:
            kind, value, title, min_val, max_val, height = self._fast
            d, lay = _BUILDERS[kind](value, title, min_val, max_val, height)
            self._data, self._layout = d, lay

    @property
    def data(self):
        self._materialize()
        self._fast = None  # the caller may mutate the tree
        return self._data

    @data.setter
    def data(self, v):
        self._materialize()
        self._fast = None
        self._data = list(v)

    @property
    def layout(self):
        self._materialize()
        self._fast = None  # the caller may mutate the tree
        return self._layout

    @layout.setter
    def layout(self, v):
        self._materialize()
        self._fast = None
        self._layout = dict(v)

    def update_layout(self, dict1=None, **kwargs):
        lay = self.layout
        if dict1:
            _merge(lay, dict1)
        if kwargs:
            _merge(lay, kwargs)
        return self

    def add_shape(self, **kwargs):
        shape = {}
        for k, v in kwargs.items():
            if "_" in k:
                _set_path(shape, k, _clean(v))
            else:
                shape[k] = _clean(v)
        self.layout.setdefault("shapes", []).append(shape)
        return self

    def to_dict(self) -> dict:
        self._materialize()
        layout = {"template": json.loads(template_json())}
        layout.update(self._layout)
        return {"data": self._data, "layout": layout}

    to_plotly_json = to_dict

    def json_parts(self) -> tuple:
        """The figure's JSON as a few strings to concatenate (no copy of the ~7 KB
        template per figure when a caller joins many figures)."""
        if self._fast is not None:
            kind, value, title, min_val, max_val, height = self._fast
            head, mid, tail = _json_template(kind, title, min_val, max_val, height)
            return head, get_color_for_value(value, max_val), mid, _value_json(value), tail
        return (self.to_json(),)

    def to_json(self) -> str:
        if self._fast is not None:
            return "".join(self.json_parts())
        body = _dumps(self._layout)
        tmpl = template_json()
        layout = '{"template":' + tmpl + ("," + body[1:] if len(body) > 2 else "}")
        return '{"data":' + _dumps(self._data) + ',"layout":' + layout + "}"

    def to_plotly(self):
        """A real ``plotly.graph_objects.Figure`` (requires Plotly)."""
        import plotly.graph_objects as go

        return go.Figure(self.to_dict())

    def __repr__(self) -> str:
        self._materialize()
        kinds = ",".join(t.get("type", "?") for t in self._data)
        return f"Figure(data=[{kinds}], layout_keys={sorted(self._layout)})"


_INF = float("inf")
_NINF = float("-inf")
_COLOR_MARK = "@@ROCMDASH_COLOR@@"
_VALUE_MARK = "@@ROCMDASH_VALUE@@"


def _value_json(value) -> str:
    if type(value) is float:  # the common case: a finite Python float
        if value == value and value not in (_INF, _NINF):
            return repr(value)
        return "null"
    v = _num(value)
    if v is None:
        return "null"
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, (int, float)):
        return repr(v)
    return json.dumps(v)


@lru_cache(maxsize=4096)
def _json_template(kind, title, min_val, max_val, height):
    """(head, mid, tail) such that head + colour + mid + value + tail is the figure's
    JSON (the colour precedes the value in both trace layouts)."""
    d, lay = _BUILDERS[kind](_VALUE_MARK, title, min_val, max_val, height, color=_COLOR_MARK)
    text = Figure(d, lay).to_json()
    c = text.index(json.dumps(_COLOR_MARK))
    v = text.index(json.dumps(_VALUE_MARK))
    assert c < v and text.count(_COLOR_MARK) == 1 and text.count(_VALUE_MARK) == 1
    return (text[:c] + '"', '"' + text[c + len(json.dumps(_COLOR_MARK)) : v], text[v + len(json.dumps(_VALUE_MARK)) :])


# ------------------------------------------------------------------------ factories
@lru_cache(maxsize=256)
def _gauge_steps(max_val):
    return tuple(
        (max_val * lo if lo else 0, max_val * hi if hi < 1.0 else max_val, GAUGE_COLORS[p])
        for (lo, hi), p in zip(((0, 0.2), (0.2, 0.4), (0.4, 0.6), (0.6, 0.8), (0.8, 1.0)), _PLATES)
    )


def _gauge_tree(value, title, min_val, max_val, height, color=None):
    color = get_color_for_value(value, max_val) if color is None else color
    steps = [{"color": c, "range": [_num(lo), _num(hi)]} for lo, hi, c in _gauge_steps(max_val)]
    trace = {
        "gauge": {
            "axis": {
                "dtick": _num(max_val / 5),
                "range": [_num(min_val), _num(max_val)],
                "showticklabels": True,
                "tick0": _num(min_val),
                "tickmode": "linear",
            },
            "bar": {"color": color, "line": {"color": "black", "width": 1}},
            "steps": steps,
        },
        "mode": "gauge+number",
        "title": {"text": title},
        "value": value if value is _VALUE_MARK else _num(value),
        "type": "indicator",
    }
    return [trace], {"margin": {"l": 30, "r": 30, "t": 0, "b": 0}, "height": _num(height)}


def _bar_tree(value, title, min_val, max_val, height, color=None):
    color = get_color_for_value(value, max_val) if color is None else color
    trace = {
        "marker": {"color": color, "line": {"color": "gray", "width": 2}},
        "orientation": "h",
        "width": 0.5,
        "x": [value if value is _VALUE_MARK else _num(value)],
        "y": [title],
        "type": "bar",
    }
    shapes = [
        {
            "fillcolor": c,
            "layer": "below",
            "line": {"width": 0},
            "opacity": 0.3,
            "type": "rect",
            "x0": _num(lo),
            "x1": _num(hi),
            "y0": -0.5,
            "y1": 0.5,
        }
        for lo, hi, c in _gauge_steps(max_val)
    ]
    layout = {
        "xaxis": {"range": [_num(min_val), _num(max_val)], "showgrid": True, "gridcolor": "lightgray"},
        "yaxis": {"showticklabels": False},
        "margin": {"l": 20, "r": 20, "t": 20, "b": 20},
        "height": _num(height),
        "showlegend": False,
        "shapes": shapes,
    }
    return [trace], layout


_BUILDERS = {"gauge": _gauge_tree, "bar": _bar_tree}


def _hashable(x) -> bool:
    try:
        hash(x)
        return True
    except TypeError:
        return False


def _make(kind, value, title, min_val, max_val, height) -> Figure:
    get_color_for_value(value, max_val)  # reference semantics: max_val == 0 raises here
    if isinstance(title, str) and _hashable(min_val) and _hashable(max_val) and _hashable(height):
        return Figure(_fast=(kind, value, title, min_val, max_val, height))
    d, lay = _BUILDERS[kind](value, title, min_val, max_val, height)
    return Figure(d, lay)


def create_gauge(value, title, min_val=0, max_val=100, height=400) -> Figure:
    """Gauge chart (app.py:70-103): 5 pastel plate steps at 20 % bands, value bar in
    the band colour with a 1 px black outline, linear ticks every max/5."""
    return _make("gauge", value, title, min_val, max_val, height)


def create_horizontal_bar(value, title, min_val=0, max_val=100, height=400) -> Figure:
    """Horizontal bar (app.py:105-151): one bar, grid on x, hidden y labels and five
    translucent background rectangles below the bar."""
    return _make("bar", value, title, min_val, max_val, height)


def panel_spec(value, title, max_val, height, use_gauge=True) -> tuple:
    """A panel as a plain tuple (kind, value, title, min_val, max_val, height): what a
    dashboard refresh keeps per chart. ``figure_from_spec`` makes the Figure on demand
    (the Streamlit page); ``spec_json_parts`` serialises it without one."""
    if max_val == 0:
        raise ZeroDivisionError("division by zero")  # as get_color_for_value(value, 0)
    return ("gauge" if use_gauge else "bar", value, title, 0, max_val, height)


def figure_from_spec(spec) -> Figure:
    kind, value, title, min_val, max_val, height = spec
    return _make(kind, value, title, min_val, max_val, height)


def spec_json_parts(spec) -> tuple:
    """Figure JSON of a panel spec as 5 strings: cached template pieces + band colour +
    value (same bytes as ``figure_from_spec(spec).to_json()``)."""
    kind, value, title, min_val, max_val, height = spec
    head, mid, tail = _json_template(kind, title, min_val, max_val, height)
    return head, get_color_for_value(value, max_val), mid, _value_json(value), tail


TREND_LINE = "#2980b9"
TREND_BAND = "rgba(41,128,185,0.25)"


def create_trend(title, age_s, lo, hi, mean, max_val=None, height=220) -> Figure:
    """A window trend (``rocmdash.ops.window_trend``) as a line over time: the slots'
    min..max as a band, their mean as a line, x = seconds before the newest sample
    (negative: time runs left to right). ``age_s`` / ``lo`` / ``hi`` / ``mean`` hold one
    entry per slot, oldest first; a slot whose age or mean is NaN (empty: no valid sample)
    becomes a null point in all three traces - a gap, never a line drawn across it.
    ``max_val``: the top of the y axis (None: autorange). No reference counterpart."""
    xs, ys = [], ([], [], [])
    for a, *v in zip(age_s, lo, hi, mean):
        a, v = _num(a), [_num(x) for x in v]
        gap = a is None or v[2] is None
        xs.append(None if a is None else -a)
        for y, x in zip(ys, v):
            y.append(None if gap else x)

    def trace(name, y, line, **more):
        return {"line": line, "mode": "lines", "name": name, "x": list(xs), "y": y, "type": "scatter", **more}

    data = [
        trace("min", ys[0], {"width": 0}, hoverinfo="skip"),
        trace("max", ys[1], {"width": 0}, fill="tonexty", fillcolor=TREND_BAND, hoverinfo="skip"),
        trace("mean", ys[2], {"color": TREND_LINE, "width": 2}),
    ]
    yaxis = {"range": [0, _num(max_val)]} if max_val is not None and _num(max_val) else {}
    layout = {
        "title": {"text": title},
        "xaxis": {"title": {"text": "seconds"}, "showgrid": True, "gridcolor": "lightgray"},
        "yaxis": yaxis,
        "margin": {"l": 40, "r": 20, "t": 40, "b": 40},
        "height": _num(height),
        "showlegend": False,
    }
    return Figure(data, layout)


QUANTILE_LINES = ("#27ae60", "#e67e22", "#c0392b")  # the lowest percentile to the highest


def create_quantiles(title, age_s, pct, values, max_val=None, height=220) -> Figure:
    """A window quantile trend (``rocmdash.ops.window_quantiles``) as three lines over the
    trend's x axis (seconds before the newest sample, negative: time runs left to right).
    ``age_s``: one entry per slot, oldest first; ``pct``: the three percentiles, naming the
    traces (``p50``); ``values``: three sequences, one per percentile, an entry per slot. A
    slot whose age or value is NaN (empty: no valid sample) is a null point - a gap, never a
    line drawn across it. ``max_val``: the top of the y axis (None: autorange). No reference
    counterpart."""
    xs = [None if _num(a) is None else -_num(a) for a in age_s]
    data = []
    for p, ys, colour in zip(pct, values, QUANTILE_LINES):
        y = [None if x is None or _num(v) is None else _num(v) for x, v in zip(xs, ys)]
        data.append({"line": {"color": colour, "width": 2}, "mode": "lines", "name": f"p{float(p):g}", "x": list(xs),
                     "y": y, "type": "scatter"})
    yaxis = {"range": [0, _num(max_val)]} if max_val is not None and _num(max_val) else {}
    layout = {
        "title": {"text": title},
        "xaxis": {"title": {"text": "seconds"}, "showgrid": True, "gridcolor": "lightgray"},
        "yaxis": yaxis,
        "margin": {"l": 40, "r": 20, "t": 40, "b": 40},
        "height": _num(height),
        "showlegend": True,
    }
    return Figure(data, layout)


def create_heatmap(title, age_s, le, counts, height=220) -> Figure:
    """A window heatmap (``rocmdash.ops.window_heatmap``) as one Plotly ``heatmap`` trace:
    x = seconds before the newest sample (negative: time runs left to right), y = each bin's
    upper bound, z = the counts. ``age_s``: one entry per slot, oldest first; ``le``: the B
    bounds; ``counts``: ``[slots][B + 1]`` per-bin counts. A slot whose age is NaN or that
    holds no valid sample (empty) is a null column - a gap, never a column of zeroes. The top
    bin (everything above the last bound, the axis maximum) has no upper bound of its own: it
    is drawn one bin width above the axis maximum and labelled ``> maximum``. No reference
    counterpart."""
    le = [_num(v) for v in le]
    B = len(le)
    step = le[-1] - le[-2] if B > 1 else (abs(le[-1]) or 1.0)
    ys = le + [le[-1] + step]
    xs, cols = [], []
    for a, c in zip(age_s, counts):
        a, c = _num(a), [int(v) for v in c]
        gap = a is None or not any(c)
        xs.append(None if a is None else -a)
        cols.append([None] * (B + 1) if gap else c)
    z = [[col[k] for col in cols] for k in range(B + 1)]  # rows of z are bins
    every = max(1, -(-B // 16))  # at most ~16 labelled bounds, and always the top bin
    ticks = list(range(every - 1, B, every))
    trace = {"colorbar": {"title": {"text": "samples"}}, "hoverongaps": False, "x": xs, "y": ys, "z": z, "zmin": 0,
             "type": "heatmap"}
    layout = {
        "title": {"text": title},
        "xaxis": {"title": {"text": "seconds"}},
        "yaxis": {"tickmode": "array", "tickvals": [ys[k] for k in ticks] + [ys[B]],
                  "ticktext": [f"{le[k]:g}" for k in ticks] + [f"> {le[-1]:g}"]},
        "margin": {"l": 40, "r": 20, "t": 40, "b": 40},
        "height": _num(height),
        "showlegend": False,
    }
    return Figure([trace], layout)


def create_autocorr(title, acf, names=None, periods=None, height=220) -> Figure:
    """A window correlogram (``rocmdash.ops.window_autocorr``) as one Plotly ``scatter`` line per
    series over the lag in samples, with a marker at each series' period. ``acf``: ``[L + 1]`` or
    ``[K][L + 1]`` (NaN: a lag without an acf, drawn as a gap); ``names``: the K trace names;
    ``periods``: per series its period in samples or None. No reference counterpart."""
    rows = [list(r) for r in acf] if len(acf) and hasattr(acf[0], "__len__") else [list(acf)]
    names = list(names) if names is not None else [f"series {k}" for k in range(len(rows))]
    periods = list(periods) if periods is not None else [None] * len(rows)
    traces = []
    for k, row in enumerate(rows):
        y = [None if v is None or v != v else _num(v) for v in row]
        traces.append({"mode": "lines", "name": names[k], "x": list(range(len(y))), "y": y, "type": "scatter"})
        p = periods[k]
        if p is not None and 0 <= int(p) < len(y) and y[int(p)] is not None:
            traces.append({"marker": {"size": 9, "symbol": "diamond"}, "mode": "markers", "name": f"{names[k]} period {int(p)}",
                           "x": [int(p)], "y": [y[int(p)]], "type": "scatter"})
    layout = {
        "title": {"text": title},
        "xaxis": {"title": {"text": "lag (samples)"}},
        "yaxis": {"range": [-1, 1], "title": {"text": "acf"}},
        "margin": {"l": 40, "r": 20, "t": 40, "b": 40},
        "height": _num(height),
        "showlegend": len(rows) > 1,
    }
    return Figure(traces, layout)


def create_periods(title, age_s, period, strength=None, height=220) -> Figure:
    """A window period trend (``rocmdash.ops.window_periods``) as one Plotly ``scatter`` trace of
    lines and markers over the trend's x axis (seconds before the newest sample, negative: time
    runs left to right): y = each slot's period in samples. ``age_s``, ``period``: one entry per
    slot, oldest first; ``strength``: the period's acf per slot, shown as the hover text and as the
    marker's opacity (0.25 at the rule's threshold of 0.5 and below, 1 at 1). A slot whose age is
    NaN or that has no period is a null point - a gap, never a line drawn across it. No reference
    counterpart."""
    xs, ys, text, alpha = [], [], [], []
    strength = list(strength) if strength is not None else [None] * len(age_s)
    for a, p, r in zip(age_s, period, strength):
        a, p, r = _num(a), _num(p), _num(r)
        gap = a is None or p is None
        xs.append(None if a is None else -a)
        ys.append(None if gap else p)
        text.append(None if gap or r is None else f"strength {r:.2f}")
        alpha.append(1.0 if gap or r is None else min(1.0, max(0.25, 0.25 + 1.5 * (r - 0.5))))
    trace = {"connectgaps": False, "marker": {"opacity": alpha, "size": 7}, "mode": "lines+markers", "name": "period",
             "text": text, "x": xs, "y": ys, "type": "scatter"}
    layout = {
        "title": {"text": title},
        "xaxis": {"title": {"text": "seconds"}, "showgrid": True, "gridcolor": "lightgray"},
        "yaxis": {"rangemode": "tozero", "title": {"text": "period (samples)"}},
        "margin": {"l": 40, "r": 20, "t": 40, "b": 40},
        "height": _num(height),
        "showlegend": False,
    }
    return Figure([trace], layout)


def create_xcorr(title, ccf, lag=None, x_name=None, y_name=None, height=220) -> Figure:
    """A window cross-correlogram (``rocmdash.ops.window_xcorr``) as one Plotly ``scatter`` line
    over the lag in samples, ``-L .. L``, with a zero line and a marker at the pair's lag.
    ``ccf``: ``[2L + 1]`` (NaN: a lag without a coefficient, drawn as a gap); ``lag``: the pair's
    lag in samples (positive: ``y_name`` follows ``x_name``) or None. No reference counterpart."""
    y = [None if v is None or v != v else _num(v) for v in ccf]
    L = len(y) // 2
    name = f"{y_name} after {x_name}" if x_name and y_name else "ccf"
    traces = [{"mode": "lines", "name": name, "x": list(range(-L, len(y) - L)), "y": y, "type": "scatter"}]
    if lag is not None and -L <= int(lag) <= L and y[L + int(lag)] is not None:
        traces.append({"marker": {"size": 9, "symbol": "diamond"}, "mode": "markers", "name": f"lag {int(lag)}",
                       "x": [int(lag)], "y": [y[L + int(lag)]], "type": "scatter"})
    layout = {
        "title": {"text": title},
        "xaxis": {"title": {"text": "lag (samples)"}},
        "yaxis": {"range": [-1, 1], "title": {"text": "r"}},
        "shapes": [{"type": "line", "x0": 0, "x1": 0, "y0": -1, "y1": 1, "line": {"width": 1, "dash": "dot"}}],
        "margin": {"l": 40, "r": 20, "t": 40, "b": 40},
        "height": _num(height),
        "showlegend": False,
    }
    return Figure(traces, layout)


def create_joint(title, le_x, le_y, counts, x_title=None, y_title=None, height=260) -> Figure:
    """A window joint histogram (``rocmdash.ops.window_joint``) as one Plotly ``heatmap`` trace:
    x = each bin's upper bound of the pair's first series, y = of its second, z = the rows in
    the cell. ``le_x`` / ``le_y``: the B bounds of the two series; ``counts``: ``[B + 1][B + 1]``
    with ``counts[i][j]`` the rows with x in bin i and y in bin j. A cell without a row is null
    - a gap, never a zero. The top bin of either axis (everything above the last bound, the axis
    maximum) is drawn as ``create_heatmap`` draws it: one bin width above the maximum and
    labelled ``> maximum``. No reference counterpart."""

    def axis(le, text):
        le = [_num(v) for v in le]
        B = len(le)
        step = le[-1] - le[-2] if B > 1 else (abs(le[-1]) or 1.0)
        vals = le + [le[-1] + step]
        every = max(1, -(-B // 16))  # at most ~16 labelled bounds, and always the top bin
        ticks = list(range(every - 1, B, every))
        ax = {"tickmode": "array", "tickvals": [vals[k] for k in ticks] + [vals[B]],
              "ticktext": [f"{le[k]:g}" for k in ticks] + [f"> {le[-1]:g}"]}
        if text is not None:
            ax["title"] = {"text": text}
        return vals, ax

    xs, xaxis = axis(le_x, x_title)
    ys, yaxis = axis(le_y, y_title)
    counts = [[int(v) for v in row] for row in counts]
    z = [[counts[i][j] or None for i in range(len(xs))] for j in range(len(ys))]  # rows of z are y bins
    trace = {"colorbar": {"title": {"text": "rows"}}, "hoverongaps": False, "x": xs, "y": ys, "z": z, "zmin": 0,
             "type": "heatmap"}
    layout = {
        "title": {"text": title},
        "xaxis": xaxis,
        "yaxis": yaxis,
        "margin": {"l": 40, "r": 20, "t": 40, "b": 40},
        "height": _num(height),
        "showlegend": False,
    }
    return Figure([trace], layout)


def create_chart(value, title, max_val, height, use_gauge=True) -> Figure:
    """Style dispatch without any UI-framework state (the app layer supplies
    ``use_gauge`` from the session, app.py:242-245)."""
    if use_gauge:
        return create_gauge(value, title, max_val=max_val, height=height)
    return create_horizontal_bar(value, title, max_val=max_val, height=height)
