"""HIP-event time of LongWindowSet.export_buckets beside export_trend over the same ring.

    python tools/probes/probe_long_buckets.py [--windows 16777216 1048576 --series 12] [--json-out FILE]

Both stream the window once, so the trend (which keeps no histogram and uses no atomics) is the
yardstick: the ratio says what the binning costs on top of the stream. One process, the two
calls alternating, one call between two events, warm, the median over the rounds. Two kinds of
rows: "iid" (every sample drawn anew: almost every sample leaves the bin of the one before, the
worst case for the kernel's run counting) and "smooth" (a slow random walk, as telemetry: long
runs inside one bucket). The buckets are checked against the refresh's counts before timing.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def rows(kind: str, n: int, S: int, rng) -> np.ndarray:
    if kind == "iid":
        x = rng.normal(50.0, 10.0, (n, S)).astype(np.float32)
    else:  # a walk that returns to where it began, so the block repeats without a jump
        step = rng.normal(0.0, 0.02, (n, S))
        walk = np.cumsum(step - step.mean(axis=0), axis=0)
        x = (50.0 + 3.0 * np.arange(S) + walk).astype(np.float32)
    x[:, ::2] = np.rint(x[:, ::2] * 4) / 4  # half the columns quantised, like readings
    return x


def main(argv=None) -> int:
    import torch

    from rocmdash.runtime import native

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, nargs="+", default=[1 << 24, 1 << 20])
    ap.add_argument("--series", type=int, default=12)
    ap.add_argument("--buckets", type=int, default=16)
    ap.add_argument("--columns", type=int, default=128)
    ap.add_argument("--kinds", nargs="+", default=["iid", "smooth"], choices=["iid", "smooth"])
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("probe_long_buckets: no GPU")
    nat = native.load()
    dev = torch.device("cuda", 0)
    S, B = args.series, args.buckets
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((S, 8), device=dev)
    bounds = np.ascontiguousarray(np.tile(np.arange(1, B + 1, dtype=np.float32) * (110.0 / B), (S, 1)))
    bd = torch.from_numpy(bounds).to(dev)
    results = []
    for W in args.windows:
        P = args.columns
        while W // P > 65536:  # the trend's limit: at most 65536 rows per column
            P *= 2
        for kind in args.kinds:
            rng = np.random.default_rng(1)
            cap = min(W, 1 << 18)
            ring = nat.SeriesRing(S, cap)
            ws = nat.LongWindowSet(W, 0)
            ws.add_ring(ring)
            block = rows(kind, cap // 2, S, rng)
            t = 0
            while t < W + 1000:  # a full window whose oldest row is not the ring's first slot
                k = min(len(block), W + 1000 - t)
                ring.push_many(block[:k], np.arange(t + 1, t + 1 + k, dtype=np.uint64))
                t += k
                ws.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
                torch.cuda.synchronize()
            trend = torch.empty((S, P + 1, 4), device=dev)
            bk = torch.empty((S, B + 1), dtype=torch.float64, device=dev)
            calls = {"export_buckets": lambda: ws.export_buckets(bd.data_ptr(), B, bk.data_ptr(), stream),
                     "export_trend": lambda: ws.export_trend(P, trend.data_ptr(), stream)}
            for f in calls.values():
                for _ in range(10):
                    f()
            torch.cuda.synchronize()
            got = bk.cpu().numpy()
            assert (got[:, B] == out.cpu().numpy()[:, 7]).all() and got[:, B].max() == W
            assert (np.diff(got, axis=1) >= 0).all()
            assert (got[:, B] == trend.cpu().numpy()[:, :, 3].astype(np.float64).sum(axis=1)).all()

            def span(f):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e3  # us

            us = {k: [] for k in calls}
            for _ in range(args.rounds):
                for k, f in calls.items():
                    us[k].append(span(f))
            nbytes = W * S * 4
            res = {"window": W, "series": S, "rows": kind, "buckets": B, "trend_columns": P, "rounds": args.rounds,
                   "bytes_streamed": nbytes, "unit": "us per call (HIP events), median"}
            for k, v in us.items():
                v = sorted(v)
                res[k] = {"p50": round(statistics.median(v), 2), "p10": round(v[len(v) // 10], 2),
                          "p90": round(v[len(v) * 9 // 10], 2), "gb_per_s": round(nbytes / statistics.median(v) / 1e3, 1)}
            res["buckets_over_trend"] = round(res["export_buckets"]["p50"] / res["export_trend"]["p50"], 3)
            print(json.dumps(res), flush=True)
            results.append(res)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
