"""Recorded behaviour of the reference dashboard (tests/golden/reference_app.json.gz): what
its app.py did on the tests' synthetic Prometheus data, written once by
tools/record_reference_golden.py from a checkout of the reference. The parity tests
compare against these records, so they need no reference checkout. Every recorded figure
carries the same plotly layout template: it is stored once (``figure_template``)."""

import gzip
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_app.json.gz")
_template = None  # the figures' common layout template, from the loaded record


def encode(x):
    """A recorded call argument as JSON: figures and data frames by content."""
    import pandas as pd

    if hasattr(x, "to_json") and hasattr(x, "to_plotly_json"):
        return {"__figure__": json.loads(x.to_json())}
    if isinstance(x, pd.DataFrame):
        return {"__dataframe__": {"index": [str(i) for i in x.index], "columns": [str(c) for c in x.columns],
                                  "data": x.to_numpy(float).tolist()}}
    if isinstance(x, pd.Series):
        return {"__series__": {"index": [str(i) for i in x.index], "index_name": x.index.name,
                               "data": [float(v) for v in x]}}
    if isinstance(x, (list, tuple)):
        return [encode(v) for v in x]
    if isinstance(x, dict):
        return {str(k): encode(v) for k, v in x.items()}
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    return {"__repr__": repr(x)}


def decode(x):
    import pandas as pd

    if isinstance(x, dict):
        if "__figure__" in x:
            fig = dict(x["__figure__"])
            fig["layout"] = dict(fig["layout"], template=_template)
            return fig
        if "__dataframe__" in x:
            d = x["__dataframe__"]
            return pd.DataFrame(d["data"], index=d["index"], columns=d["columns"])
        if "__series__" in x:
            s = x["__series__"]
            return pd.Series(s["data"], index=pd.Index(s["index"], name=s["index_name"]))
        return {k: decode(v) for k, v in x.items()}
    if isinstance(x, list):
        return [decode(v) for v in x]
    return x


def encode_calls(calls):
    return [[name, [encode(a) for a in args], {k: encode(v) for k, v in kwargs.items()}] for name, args, kwargs in calls]


def decode_calls(calls):
    return [(name, tuple(decode(a) for a in args), {k: decode(v) for k, v in kwargs.items()})
            for name, args, kwargs in calls]


def save(record):
    """Write the record, the figures' one template factored out of them."""
    templates = []

    def strip(x):
        if isinstance(x, dict):
            if "__figure__" in x:
                templates.append(x["__figure__"]["layout"].pop("template"))
            for v in x.values():
                strip(v)
        elif isinstance(x, list):
            for v in x:
                strip(v)

    strip(record)
    assert templates and all(t == templates[0] for t in templates), "figures with different templates"
    record = dict(record, figure_template=templates[0])
    with open(GOLDEN, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
        f.write(json.dumps(record, separators=(",", ":"), sort_keys=True).encode())


def load():
    global _template
    with gzip.open(GOLDEN, "rt") as f:
        record = json.load(f)
    _template = record["figure_template"]
    return record
