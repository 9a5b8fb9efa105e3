"""HIP-event time of export_excursions (K thresholds) beside export_trend over the same rings
in the same process: the trend's order-free stream of the same bytes is the yardstick.

    python tools/bench_window_excursions.py [--window 4096 --series 16] [--json-out FILE]
    python tools/bench_window_excursions.py --long --window 16777216 --series 12 [--rows independent]

One call between two events, warm, the median over the rounds, and 20 calls back to back
between two events divided by 20. ``--rows telemetry``: slow random walks, half the columns
integer-valued, like readings (long episodes); ``--rows independent``: every sample drawn on
its own (an episode boundary every other sample). The records are checked against the
reference (short windows: every integer; long ones: against the set's own valid counts).
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

    from rocmdash.ops.window_excursions import E_VALID, window_excursions_reference
    from rocmdash.runtime import native

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--series", type=int, default=16)
    ap.add_argument("--thresholds", type=int, default=3)
    ap.add_argument("--columns", type=int, default=None, help="the trend's columns (default: 128, or window / 32768 if more)")
    ap.add_argument("--long", action="store_true", help="a LongWindowSet (windows of 2^10 .. 2^26 rows)")
    ap.add_argument("--rows", choices=["telemetry", "independent"], default="telemetry")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_excursions: no GPU")
    nat = native.load()
    dev = torch.device("cuda", 0)
    W, S, K = args.window, args.series, args.thresholds
    P = args.columns or max(128, W // 32768)
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((S, 8), device=dev)
    trend = torch.empty((S, P + 1, 4), device=dev)
    dst = torch.full((S, K, 8), -1, dtype=torch.int32, device=dev)
    nbytes_work = nat.excursion_workspace_bytes(S, K)
    work = torch.empty(nbytes_work, dtype=torch.uint8, device=dev)
    # thresholds at 50 / 75 / 90 / 95 % of an axis of 100, rows around 50 +- 20
    thr = np.tile(np.array([50.0, 75.0, 90.0, 95.0][:K], np.float32), (S, 1))
    td = torch.from_numpy(thr).to(dev)
    rng = np.random.default_rng(0)

    def rows(k):
        if args.rows == "independent":
            return rng.normal(50.0, 20.0, (k, S)).astype(np.float32)
        x = 50.0 + np.cumsum(rng.normal(0.0, 0.5, (k, S)), axis=0)
        x = 50.0 + 40.0 * np.sin((x - 50.0) / 40.0)  # a bounded walk: stays within 10 .. 90
        x = x.astype(np.float32)
        x[:, ::2] = np.rint(x[:, ::2])
        return x

    if args.long:
        cap = min(W, 1 << 18)
        ring = nat.SeriesRing(S, cap)
        ws = nat.LongWindowSet(W, 0)
        ws.add_ring(ring)
        block = rows(cap // 2)
        t = 0
        while t < W + W // 8:  # a full window that wraps the device ring
            k = min(len(block), W + W // 8 - t)
            ring.push_many(block[:k], np.arange(t + 1, t + 1 + k, dtype=np.uint64))
            t += k
            ws.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
            torch.cuda.synchronize()
    else:
        ring = nat.SeriesRing(S, 4 * W)
        ws = nat.DeviceWindowSet(W, 0)
        ws.add_ring(ring)
        x = rows(W + W // 8)
        t = len(x)
        ring.push_many(x, np.arange(1, t + 1, dtype=np.uint64))
        ws.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
        torch.cuda.synchronize()

    calls = {"export_excursions": lambda: ws.export_excursions(td.data_ptr(), K, dst.data_ptr(), work.data_ptr(),
                                                               nbytes_work, stream),
             "export_trend": lambda: ws.export_trend(P, trend.data_ptr(), stream)}
    for f in calls.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:, :, 7] == W).all() and (got[:, 0, E_VALID] == out.cpu().numpy()[:, 7]).all()
    if not args.long:  # small enough to check every integer here
        assert np.array_equal(got, window_excursions_reference(ring.window(W)[0], thr))

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
    res = {"set": "LongWindowSet" if args.long else "DeviceWindowSet", "window": W, "series": S, "thresholds": K,
           "trend_columns": P, "rows": args.rows, "rounds": args.rounds, "bytes_streamed": nbytes,
           "chunk_rows": int(nat.excursion_plan_chunk_rows(W)), "episodes_first_series": got[0, :, 2].tolist(),
           "unit": "us per call (HIP events)"}
    for k in calls:
        v = sorted(single[k])
        res[k] = {"single_p50": round(statistics.median(v), 2), "single_p10": round(v[len(v) // 10], 2),
                  "single_p90": round(v[len(v) * 9 // 10], 2), "back_to_back_mean": round(statistics.mean(batch[k]), 2),
                  "back_to_back_min": round(min(batch[k]), 2)}
    for m in ("single_p50", "back_to_back_mean"):
        res[f"excursions_over_trend_{m}"] = round(res["export_excursions"][m] / res["export_trend"][m], 3)
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
