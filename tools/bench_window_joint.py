"""HIP-event time of export_joint (K pairs x B buckets per axis) beside export_buckets and
export_trend over the same ring in the same process: all three stream the same bytes once, so
the buckets' time on the same ring is the yardstick.

    python tools/bench_window_joint.py [--window 4096 --series 16] [--json-out FILE]
    python tools/bench_window_joint.py --long --window 16777216 --series 12 [--rows independent]

The result is verified first: every cell against the reference, and the row and column sums of
each pair against the de-cumulated export_buckets counts of its two series (the rows hold no
NaN). Then one call between two events, warm, the median over the rounds, and 20 calls back to
back between two events divided by 20, the three exports alternating. ``--rows telemetry``:
slow bounded random walks, half the columns integer-valued, like readings (long runs inside one
cell); ``--rows independent``: every sample drawn on its own (a new cell nearly every row).
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

    from rocmdash.ops.window_joint import window_joint_reference
    from rocmdash.runtime import native

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--series", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=4, help="K: the first K of eight fixed pairs")
    ap.add_argument("--buckets", type=int, default=16)
    ap.add_argument("--columns", type=int, default=64, help="of the trend beside it")
    ap.add_argument("--long", action="store_true", help="a LongWindowSet (windows of 2^10 .. 2^26 rows)")
    ap.add_argument("--rows", choices=["telemetry", "independent"], default="telemetry")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_joint: no GPU")
    nat = native.load()
    dev = torch.device("cuda", 0)
    W, S, K, B, P = args.window, args.series, args.pairs, args.buckets, args.columns
    if S < 8 or not 1 <= K <= 8:
        raise SystemExit("bench_window_joint: at least 8 series, 1 to 8 pairs")
    # integer-valued with continuous columns, a pair and its transpose from the fifth on
    pairs = [(0, 1), (2, 3), (4, 6), (7, 5), (1, 0), (3, 2), (0, 2), (1, 7)][:K]
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((S, 8), device=dev)
    trend = torch.empty((S, P + 1, 4), device=dev)
    buckets = torch.empty((S, B + 1), dtype=torch.float64 if args.long else torch.float32, device=dev)
    dst = torch.full((K, B + 1, B + 1), -1, dtype=torch.int32, device=dev)
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

    total = W + 1000  # a full window in a wrapped device ring
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

    calls = {"export_joint": lambda: ws.export_joint(pairs, bd.data_ptr(), B, dst.data_ptr(), stream),
             "export_buckets": lambda: ws.export_buckets(bd.data_ptr(), B, buckets.data_ptr(), stream),
             "export_trend": lambda: ws.export_trend(P, trend.data_ptr(), stream)}
    for f in calls.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    # the window is rows [t - W, t) of the stream; every row of the block is in it equally often
    # when W is a multiple of the block (a long window)
    if W % len(block) == 0:
        want = window_joint_reference(block, pairs, bounds).astype(np.int64) * (W // len(block))
    else:
        want = window_joint_reference(block[np.arange(t - W, t) % len(block)], pairs, bounds)
    assert np.array_equal(got, want), "export_joint differs from the reference"
    marg = np.diff(np.concatenate([np.zeros((S, 1)), buckets.cpu().numpy().astype(np.float64)], axis=1), axis=1)
    for k, (a, b) in enumerate(pairs):
        assert (got[k].sum(axis=1) == marg[a]).all() and (got[k].sum(axis=0) == marg[b]).all(), f"pair {k}"

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
    res = {"set": "LongWindowSet" if args.long else "DeviceWindowSet", "window": W, "series": S, "pairs": pairs,
           "buckets": B, "trend_columns": P, "rows": args.rows, "rounds": args.rounds, "bytes_streamed": nbytes,
           "nonzero_cells": [int(np.count_nonzero(g)) for g in got], "verified": True, "unit": "us per call (HIP events)"}
    for k in calls:
        v = sorted(single[k])
        res[k] = {"single_p50": round(statistics.median(v), 2), "single_p10": round(v[len(v) // 10], 2),
                  "single_p90": round(v[len(v) * 9 // 10], 2), "back_to_back_mean": round(statistics.mean(batch[k]), 2),
                  "back_to_back_min": round(min(batch[k]), 2)}
    for m in ("single_p50", "back_to_back_mean"):
        res[f"joint_over_buckets_{m}"] = round(res["export_joint"][m] / res["export_buckets"][m], 3)
        res[f"joint_over_trend_{m}"] = round(res["export_joint"][m] / res["export_trend"][m], 3)
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
