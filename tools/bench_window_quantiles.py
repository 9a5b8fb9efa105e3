"""HIP-event time of export_quantiles beside export_trend over the same rings, in the same
process, alternating: a short window set, or a long window set's whole-window stream.

    python tools/bench_window_quantiles.py [--window 4096 --series 16 --columns 64] [--json-out FILE]
    python tools/bench_window_quantiles.py --long --window 16777216 --series 12 --columns 512 [--rows independent]

One call between two events, warm, the median over the rounds (on an idle GPU that span
includes the launch's own start-up), and 20 calls of each export back to back between two
events divided by 20, the two exports alternating. ``--rows telemetry``: slow bounded random
walks, half the columns integer-valued, like readings (neighbouring samples share their high
digits); ``--rows independent``: every sample drawn on its own. The export is checked before
it is timed: its counts against the trend's, and some slots (all of them for a short window)
against the numpy reference.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    import torch

    from rocmdash.ops.window_quantiles import window_quantiles_reference
    from rocmdash.ops.window_trend import check_columns, trend_geometry
    from rocmdash.runtime import native

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--series", type=int, default=16)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--long", action="store_true", help="a LongWindowSet (windows of 2^10 .. 2^26 rows)")
    ap.add_argument("--rows", choices=["telemetry", "independent"], default="telemetry")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_quantiles: no GPU")
    nat = native.load()
    dev = torch.device("cuda", 0)
    W, S, P = args.window, args.series, args.columns
    c = check_columns(P, W)
    pct = (50.0, 90.0, 99.0)
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((S, 8), device=dev)
    trend = torch.empty((S, P + 1, 4), device=dev)
    dst = torch.full((S, P + 1, 4), -1.0, device=dev)
    rng = np.random.default_rng(0)

    def rows(k):
        if args.rows == "independent":
            return rng.normal(50.0, 20.0, (k, S)).astype(np.float32)
        x = 50.0 + np.cumsum(rng.normal(0.0, 0.5, (k, S)), axis=0)
        x = 50.0 + 40.0 * np.sin((x - 50.0) / 40.0)  # a bounded walk: stays within 10 .. 90
        x = x.astype(np.float32)
        x[:, ::2] = np.rint(x[:, ::2])
        return x

    total = W + c // 2  # a full window whose newest column is half full (and a wrapped device ring)
    if args.long:
        cap = min(W, 1 << 18)
        ring = nat.SeriesRing(S, cap)
        ws = nat.LongWindowSet(W, 0)
        ws.add_ring(ring)
        block = rows(cap // 2)  # row r of the stream is block[r % len(block)]
        t = 0
        while t < total:
            k = min(len(block), total - t)
            ring.push_many(block[:k], np.arange(t + 1, t + 1 + k, dtype=np.uint64))
            t += k
            ws.refresh(out.data_ptr(), stream, *pct)
            torch.cuda.synchronize()
    else:
        ring = nat.SeriesRing(S, 4 * W)
        ws = nat.DeviceWindowSet(W, 0)
        ws.add_ring(ring)
        block = rows(total)
        t = total
        ring.push_many(block, np.arange(1, t + 1, dtype=np.uint64))
        ws.refresh(out.data_ptr(), stream, *pct)
        torch.cuda.synchronize()

    calls = {"export_quantiles": lambda: ws.export_quantiles(P, dst.data_ptr(), stream, *pct),
             "export_trend": lambda: ws.export_trend(P, trend.data_ptr(), stream)}
    for f in calls.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    got, tr = dst.cpu().numpy(), trend.cpu().numpy()
    assert np.array_equal(got[:, :, 3], tr[:, :, 3])
    _, ranges = trend_geometry(t, W, W, P)
    for j in sorted({0, 1, P // 2, P - 1, P} if args.long else set(range(P + 1))):
        lo, hi = (int(v) for v in ranges[j])
        if hi <= lo:
            assert (got[:, j, 3] == 0).all() and np.isnan(got[:, j, :3]).all(), f"slot {j}"
            continue
        x = block[np.arange(lo, hi) % len(block)]
        want = window_quantiles_reference(x, hi, W, P, pct)  # rows [lo, hi) alone: its last slot is column j
        assert np.array_equal(got[:, j, 3], want[:, P, 3]), f"slot {j}: count"
        # the interpolation may be contracted into an fma on the device: one fp32 ulp
        assert (np.abs(got[:, j, :3] - want[:, P, :3]) <= np.spacing(np.abs(want[:, P, :3]))).all(), f"slot {j}"

    def span(f, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / k  # us per call

    single = {k: [] for k in calls}
    batch = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, f in calls.items():
            single[k].append(span(f, 1))
    for _ in range(max(1, args.rounds // 20)):
        for k, f in calls.items():
            batch[k].append(span(f, 20))
    nbytes = W * S * 4
    res = {"set": "LongWindowSet" if args.long else "DeviceWindowSet", "window": W, "series": S, "columns": P,
           "rows_per_column": c, "path": "select" if c > nat.QUANTILE_SORT_MAX_ROWS else "sort", "rows": args.rows,
           "rounds": args.rounds, "window_bytes": nbytes, "verified": True, "unit": "us per call (HIP events)"}
    for k in calls:
        v = sorted(single[k])
        res[k] = {"single_p50": round(statistics.median(v), 2), "single_p10": round(v[len(v) // 10], 2),
                  "single_p90": round(v[len(v) * 9 // 10], 2), "back_to_back_mean": round(statistics.mean(batch[k]), 2),
                  "back_to_back_min": round(min(batch[k]), 2)}
    for m in ("single_p50", "back_to_back_mean"):
        res[f"quantiles_over_trend_{m}"] = round(res["export_quantiles"][m] / res["export_trend"][m], 3)
    line = json.dumps(res)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
