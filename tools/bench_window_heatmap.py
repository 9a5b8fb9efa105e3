"""HIP-event time of export_heatmap (P columns x B buckets) beside export_trend over the same
rings in the same process: both stream the same bytes once, so their ratio is the figure.

    python tools/bench_window_heatmap.py [--window 4096 --series 16 --columns 64] [--json-out FILE]
    python tools/bench_window_heatmap.py --long --window 16777216 --series 12 --columns 512 [--rows independent]

The result is verified first: every count against the reference for a short window; for a
long one the first, the last and three other slots against the reference, every slot's bins
against the trend's count and the slots summed and cumulated against export_buckets. Then one
call between two events, warm, the median over the rounds, and 20 calls back to back between
two events divided by 20, the two exports alternating. ``--rows telemetry``: slow bounded
random walks, half the columns integer-valued, like readings (long runs inside one bucket);
``--rows independent``: every sample drawn on its own (a new bucket nearly every sample).
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

    from rocmdash.ops.window_heatmap import window_heatmap_reference
    from rocmdash.ops.window_trend import check_columns, trend_geometry
    from rocmdash.runtime import native

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--series", type=int, default=16)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--buckets", type=int, default=16)
    ap.add_argument("--long", action="store_true", help="a LongWindowSet (windows of 2^10 .. 2^26 rows)")
    ap.add_argument("--rows", choices=["telemetry", "independent"], default="telemetry")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_heatmap: no GPU")
    nat = native.load()
    dev = torch.device("cuda", 0)
    W, S, P, B = args.window, args.series, args.columns, args.buckets
    c = check_columns(P, W)
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((S, 8), device=dev)
    trend = torch.empty((S, P + 1, 4), device=dev)
    dst = torch.full((S, P + 1, B + 1), -1, dtype=torch.int32, device=dev)
    # evenly spaced bounds up to an axis of 100 (the default bounds' shape), rows around 50
    bounds = np.tile((np.arange(1, B + 1, dtype=np.float64) * 100.0 / B).astype(np.float32), (S, 1))
    bd = torch.from_numpy(bounds).to(dev)
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
            ws.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
            torch.cuda.synchronize()
    else:
        ring = nat.SeriesRing(S, 4 * W)
        ws = nat.DeviceWindowSet(W, 0)
        ws.add_ring(ring)
        block = rows(total)
        t = total
        ring.push_many(block, np.arange(1, t + 1, dtype=np.uint64))
        ws.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
        torch.cuda.synchronize()

    calls = {"export_heatmap": lambda: ws.export_heatmap(P, bd.data_ptr(), B, dst.data_ptr(), stream),
             "export_trend": lambda: ws.export_trend(P, trend.data_ptr(), stream)}
    for f in calls.values():
        for _ in range(10):
            f()
    buckets = torch.empty((S, B + 1), dtype=torch.float64 if args.long else torch.float32, device=dev)
    ws.export_buckets(bd.data_ptr(), B, buckets.data_ptr(), stream)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got.sum(axis=2) == trend.cpu().numpy()[:, :, 3]).all()
    assert (np.cumsum(got.sum(axis=1), axis=1) == buckets.cpu().numpy()).all()
    _, ranges = trend_geometry(t, W, W, P)
    for j in sorted({0, 1, P // 2, P - 1, P} if args.long else set(range(P + 1))):
        lo, hi = (int(v) for v in ranges[j])
        x = block[np.arange(lo, hi) % len(block)]
        want = window_heatmap_reference(x, hi, W, P, bounds)  # rows [lo, hi) alone: its last slot is column j
        assert np.array_equal(got[:, j], want[:, P]) and want[:, :P].sum() == 0, f"slot {j}"

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
           "buckets": B, "rows_per_column": c, "rows": args.rows, "rounds": args.rounds, "bytes_streamed": nbytes,
           "verified": True, "unit": "us per call (HIP events)"}
    for k in calls:
        v = sorted(single[k])
        res[k] = {"single_p50": round(statistics.median(v), 2), "single_p10": round(v[len(v) // 10], 2),
                  "single_p90": round(v[len(v) * 9 // 10], 2), "back_to_back_mean": round(statistics.mean(batch[k]), 2),
                  "back_to_back_min": round(min(batch[k]), 2)}
    for m in ("single_p50", "back_to_back_mean"):
        res[f"heatmap_over_trend_{m}"] = round(res["export_heatmap"][m] / res["export_trend"][m], 3)
        res[f"gb_per_s_{m}"] = {k: round(nbytes / res[k][m] / 1e3, 1) for k in calls}
    line = json.dumps(res)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
