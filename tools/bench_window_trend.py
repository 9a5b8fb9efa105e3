"""HIP-event time of export_trend: a short window set beside the empty-kernel floor on the
same grid, or a long window set's whole-window stream (bytes streamed and implied GB/s).

    python tools/bench_window_trend.py [--window 4096 --series 16 --columns 128] [--json-out FILE]
    python tools/bench_window_trend.py --long --window 16777216 --series 12 --columns 512

One call between two events, warm, the median over the rounds (on an idle GPU that span
includes the launch's own start-up), and 100 calls back to back between two events divided
by 100. The long window is filled with generated telemetry-like rows, ring-full by ring-full.
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

    from rocmdash.ops.window_trend import check_columns, window_trend_reference
    from rocmdash.runtime import native

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--series", type=int, default=16)
    ap.add_argument("--columns", type=int, default=128)
    ap.add_argument("--long", action="store_true", help="a LongWindowSet (windows of 2^10 .. 2^26 rows)")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_trend: no GPU")
    nat = native.load()
    dev = torch.device("cuda", 0)
    W, S, P = args.window, args.series, args.columns
    c = check_columns(P, W)
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((S, 8), device=dev)
    dst = torch.empty((S, P + 1, 4), device=dev)
    rng = np.random.default_rng(0)
    if args.long:
        cap = min(W, 1 << 18)
        ring = nat.SeriesRing(S, cap)
        ws = nat.LongWindowSet(W, 0)
        ws.add_ring(ring)
        block = rng.normal(50.0, 10.0, (cap // 2, S)).astype(np.float32)
        block[:, ::2] = np.rint(block[:, ::2])  # half the columns integer-valued, like readings
        t = 0
        while t < W + c // 2:  # a full window whose newest column is half full
            k = min(len(block), W + c // 2 - t)
            ring.push_many(block[:k], np.arange(t + 1, t + 1 + k, dtype=np.uint64))
            t += k
            ws.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
            torch.cuda.synchronize()
    else:
        ring = nat.SeriesRing(S, 4 * W)
        ws = nat.DeviceWindowSet(W, 0)
        ws.add_ring(ring)
        x = rng.normal(50.0, 20.0, (W + c // 2, S)).astype(np.float32)
        t = len(x)
        ring.push_many(x, np.arange(1, t + 1, dtype=np.uint64))
        ws.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
        torch.cuda.synchronize()

    grid = P + 1  # the workgroups of the floor: one per slot, each gone after one clock read
    calls = {"export_trend": lambda: ws.export_trend(P, dst.data_ptr(), stream),
             "empty_kernel": lambda: nat.spin(grid, 0.01, stream)}
    for f in calls.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert got[:, :, 3].sum(axis=1).max() == W and (got[:, :, 3].sum(axis=1) == out.cpu().numpy()[:, 7]).all()
    if not args.long:  # small enough to check every slot here
        want = window_trend_reference(ring.window(W)[0], t, W, P)
        assert np.array_equal(got[:, :, [0, 1, 3]], want[:, :, [0, 1, 3]], equal_nan=True)

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
            batch[k].append(span(f, 100))
    nbytes = W * S * 4
    res = {"set": "LongWindowSet" if args.long else "DeviceWindowSet", "window": W, "series": S, "columns": P,
           "rows_per_column": c, "rounds": args.rounds, "bytes_streamed": nbytes, "unit": "us per call (HIP events)"}
    for k in calls:
        v = sorted(single[k])
        res[k] = {"single_p50": round(statistics.median(v), 2), "single_p10": round(v[len(v) // 10], 2),
                  "single_p90": round(v[len(v) * 9 // 10], 2), "back_to_back_mean": round(statistics.mean(batch[k]), 2),
                  "back_to_back_min": round(min(batch[k]), 2)}
    res["gb_per_s"] = {m: round(nbytes / res["export_trend"][m] / 1e3, 1) for m in ("single_p50", "back_to_back_mean")}
    line = json.dumps(res)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
