#!/usr/bin/env python3
"""Record what the reference dashboard's app.py does on the parity tests' synthetic
Prometheus data into tests/golden/reference_app.json.gz (tests/_golden.py), so the tests
run without a reference checkout.

    python tools/record_reference_golden.py --reference /path/to/reference/app.py

Run it again only when the tests' inputs (node sizes, seeds, faults) change."""

import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "stubs")]


class _Stop(Exception):
    pass


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reference", required=True, help="the reference checkout's app.py")
    args = ap.parse_args()

    import streamlit as st  # the recording double (tests/stubs)

    import _golden
    from test_app import PAGE_CASES, page_case
    from test_query import FAULTS, fault_case

    from rocmdash.prom.mock import FakePrometheusHTTP, SyntheticNode

    spec = importlib.util.spec_from_file_location("reference_app", args.reference)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"podname": ref.PROMETHEUS_METRICS_PODNAME}

    # the two PromQL strings the reference sends
    sent = []
    fake = FakePrometheusHTTP(SyntheticNode(2, host_ip="10.1.2.3"))

    def get(url=None, params=None, **kw):
        sent.append(params["query"])
        return fake(url=url, params=params)

    ref.requests.get = get
    ref.fetch_gpu_metrics()
    out["queries_sent"] = sent[:2]

    # fetch_gpu_metrics on the parity node
    ref.requests.get = FakePrometheusHTTP(SyntheticNode(8, seed=3))
    df, stats = ref.fetch_gpu_metrics()
    num = [c for c in df.columns if c != "card_model"]
    out["fetch"] = {"index": [str(i) for i in df.index], "columns": list(df.columns),
                    "card_model": [str(v) for v in df["card_model"]],
                    "numeric": {c: [float(v) for v in df[c].astype(float)] for c in num},
                    "stats": {k: _golden.encode(stats[k].astype(float)) for k in ("mean", "max", "min")}}

    # the error paths
    out["faults"] = {}
    for fault in FAULTS:
        node, kw = fault_case(fault)
        ref.requests.get = FakePrometheusHTTP(node, **kw)
        out["faults"][fault] = _golden.encode(list(ref.fetch_gpu_metrics()))

    # the page
    def stop(_):
        raise _Stop()

    ref.time.sleep = stop
    out["page"] = {}
    for select_all, gauge in PAGE_CASES:
        node, widgets = page_case(select_all, gauge)
        ref.requests.get = FakePrometheusHTTP(node)
        st.reset()
        st.WIDGET_VALUES.update(widgets)
        try:
            ref.main()
        except _Stop:
            pass
        out["page"][f"{int(select_all)}-{int(gauge)}"] = _golden.encode_calls(list(st.CALLS))
    _golden.save(out)
    print(f"wrote {_golden.GOLDEN} ({os.path.getsize(_golden.GOLDEN)} bytes)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
