"""HIP-event time of export_autocorr (lags 0 .. L over the newest SPAN rows) beside export_trend
over the same ring in the same process. The trend streams the ring once; the autocorrelation does
``series x N x (L + 1)`` pair-products on top, so its time is reported as pair-products per second
and as a ratio to the trend's.

    python tools/bench_window_autocorr.py [--window 4096 --series 16 --lags 64] [--json-out FILE]
    python tools/bench_window_autocorr.py --long --window 65536 --series 12 --lags 512 [--rows independent] [--nan 0.01]
    python tools/bench_window_autocorr.py --long --window 1048576 --span 1048576 --series 12 --lags 1024

The result is verified first, every word against the reference (for N x L above 2^27 on a sample
of the lags, through the one-lag sums). Then one call between two events, warm, the median over
the rounds, and 20 calls back to back between two events divided by 20, the two exports
alternating. ``--rows telemetry``: slow bounded random walks, half the columns integer-valued,
like readings; ``--rows independent``: every sample drawn on its own. ``--nan F``: that share of
the samples is NaN, so most chunks run the loop for all four sums.
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

    from rocmdash.ops.window_autocorr import check_autocorr, quantise, window_autocorr_reference
    from rocmdash.runtime import native

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--series", type=int, default=16)
    ap.add_argument("--lags", type=int, default=64)
    ap.add_argument("--span", type=int, default=65536)
    ap.add_argument("--columns", type=int, default=64, help="of the trend beside it")
    ap.add_argument("--long", action="store_true", help="a LongWindowSet (windows of 2^10 .. 2^26 rows)")
    ap.add_argument("--rows", choices=["telemetry", "independent"], default="telemetry")
    ap.add_argument("--nan", type=float, default=0.0, help="share of NaN samples")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_autocorr: no GPU")
    nat = native.load()
    dev = torch.device("cuda", 0)
    W, S, P = args.window, args.series, args.columns
    L, span = check_autocorr(args.lags, args.span, W)
    N = min(W, span)
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((S, 8), device=dev)
    trend = torch.empty((S, P + 1, 4), device=dev)
    dst = torch.full((S, L + 1, 4), -1, dtype=torch.int64, device=dev)
    scale = np.full(S, np.float32(4095.0 / 100.0), np.float32)  # an axis of 100, rows around 50
    sd = torch.from_numpy(scale).to(dev)
    rng = np.random.default_rng(0)

    def rows(k):
        if args.rows == "independent":
            x = rng.normal(50.0, 20.0, (k, S)).astype(np.float32)
        else:
            x = 50.0 + np.cumsum(rng.normal(0.0, 0.5, (k, S)), axis=0)
            x = 50.0 + 40.0 * np.sin((x - 50.0) / 40.0)  # a bounded walk: stays within 10 .. 90
            x = x.astype(np.float32)
            x[:, ::2] = np.rint(x[:, ::2])
        if args.nan > 0:
            x[rng.random((k, S)) < args.nan] = np.nan
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

    calls = {"export_autocorr": lambda: ws.export_autocorr(span, sd.data_ptr(), L, dst.data_ptr(), stream),
             "export_trend": lambda: ws.export_trend(P, trend.data_ptr(), stream)}
    for f in calls.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    newest = block[np.arange(t - N, t) % len(block)]  # the span: rows [t - N, t) of the stream
    if N * L <= 1 << 27:
        assert np.array_equal(got, window_autocorr_reference(newest, scale, L, span)), "export_autocorr differs from the reference"
        checked = L + 1
    else:  # the same sums, one lag at a time, for a sample of the lags
        q, v = quantise(newest, scale)
        lags = sorted({0, 1, 2, 7, 8, 255, 256, 257, L // 2, L - 1, L})
        for k in lags:
            q0, v0, qk, vk = q[: N - k], v[: N - k], q[k:], v[k:]
            want = np.stack([(v0 * vk).sum(0), (q0 * vk).sum(0), (v0 * qk).sum(0), (q0 * qk).sum(0)], axis=1)
            assert np.array_equal(got[:, k], want), f"export_autocorr differs from the reference at lag {k}"
        checked = len(lags)

    def timed(f, k):
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
            single[k].append(timed(f, 1))
    for _ in range(max(1, args.rounds // 20)):
        for k, f in calls.items():
            batch[k].append(timed(f, 20))
    products = S * N * (L + 1)
    res = {"set": "LongWindowSet" if args.long else "DeviceWindowSet", "window": W, "span_rows": N, "series": S, "lags": L,
           "trend_columns": P, "rows": args.rows, "nan": args.nan, "rounds": args.rounds, "pair_products": products,
           "lags_verified": checked, "verified": True, "unit": "us per call (HIP events)"}
    for k in calls:
        v = sorted(single[k])
        res[k] = {"single_p50": round(statistics.median(v), 2), "single_p10": round(v[len(v) // 10], 2),
                  "single_p90": round(v[len(v) * 9 // 10], 2), "back_to_back_mean": round(statistics.mean(batch[k]), 2),
                  "back_to_back_min": round(min(batch[k]), 2)}
    for m in ("single_p50", "back_to_back_mean"):
        res[f"autocorr_over_trend_{m}"] = round(res["export_autocorr"][m] / res["export_trend"][m], 3)
        res[f"giga_pair_products_per_s_{m}"] = round(products / res["export_autocorr"][m] / 1e3, 1)
    line = json.dumps(res)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
