"""HIP-event time of export_xcorr (K pairs, lags -L .. L over the newest SPAN rows) beside
export_autocorr (every series, lags 0 .. L) over the same ring in the same process. Both are
multiply-adds over ``rows x lags``: a pair costs ``N x (2L + 1)`` pair-products (and six sums), a
series of the autocorrelation ``N x (L + 1)`` (and four), so both times are reported as
pair-products per second - the autocorrelation's rate of the same run is the yardstick.

    python tools/bench_window_xcorr.py [--window 4096 --series 16 --lags 64] [--json-out FILE]
    python tools/bench_window_xcorr.py --long --window 65536 --series 12 --lags 255 [--rows independent] [--nan 0.01]
    python tools/bench_window_xcorr.py --long --window 1048576 --span 1048576 --series 12 --lags 1024

The result is verified first, every word against the reference (for N x L above 2^22 on a sample
of the lags, through the one-lag sums). Then one call between two events, warm, the median over
the rounds, and 20 calls back to back between two events divided by 20, the two exports
alternating. ``--rows telemetry``: slow bounded random walks, half the columns integer-valued,
like readings; ``--rows independent``: every sample drawn on its own. ``--nan F``: that share of
the samples is NaN, so most chunks run the loop for all six sums.
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

    from rocmdash.ops.window_autocorr import quantise
    from rocmdash.ops.window_xcorr import check_pairs, check_xcorr, window_xcorr_reference
    from rocmdash.runtime import native

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--series", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=4, help="K: pair i is (i, series - 1 - i)")
    ap.add_argument("--lags", type=int, default=64)
    ap.add_argument("--span", type=int, default=65536)
    ap.add_argument("--long", action="store_true", help="a LongWindowSet (windows of 2^10 .. 2^26 rows)")
    ap.add_argument("--rows", choices=["telemetry", "independent"], default="telemetry")
    ap.add_argument("--nan", type=float, default=0.0, help="share of NaN samples")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_xcorr: no GPU")
    nat = native.load()
    dev = torch.device("cuda", 0)
    W, S, K = args.window, args.series, args.pairs
    L, span = check_xcorr(args.lags, args.span, W)
    pairs = check_pairs([(i, S - 1 - i) for i in range(K)], S)
    N = min(W, span)
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((S, 8), device=dev)
    auto = torch.full((S, L + 1, 4), -1, dtype=torch.int64, device=dev)
    dst = torch.full((K, 2 * L + 1, 6), -1, dtype=torch.int64, device=dev)
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

    calls = {"export_xcorr": lambda: ws.export_xcorr(pairs, span, sd.data_ptr(), L, dst.data_ptr(), stream),
             "export_autocorr": lambda: ws.export_autocorr(span, sd.data_ptr(), L, auto.data_ptr(), stream)}
    for f in calls.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    newest = block[np.arange(t - N, t) % len(block)]  # the span: rows [t - N, t) of the stream
    if N * L <= 1 << 22:
        assert np.array_equal(got, window_xcorr_reference(newest, pairs, scale, L, span)), "export_xcorr differs from the reference"
        checked = 2 * L + 1
    else:  # the same sums, one lag at a time, for a sample of the lags
        q, v = quantise(newest, scale)
        lags = sorted({s * k for s in (-1, 1) for k in (0, 1, 2, 7, 8, 255, 256, 257, L // 2, L - 1, L) if k <= L})
        for k in lags:
            t0, t1 = max(0, -k), min(N, N - k)
            for i, (a, b) in enumerate(pairs):
                qa, va, qb, vb = q[t0:t1, a], v[t0:t1, a], q[t0 + k : t1 + k, b], v[t0 + k : t1 + k, b]
                want = [(va * vb).sum(), (qa * vb).sum(), (va * qb).sum(), (qa * qb).sum(), (qa * qa * vb).sum(), (va * qb * qb).sum()]
                assert got[i, L + k].tolist() == want, f"export_xcorr differs from the reference at pair {i}, lag {k}"
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
    products = {"export_xcorr": K * N * (2 * L + 1), "export_autocorr": S * N * (L + 1)}
    res = {"set": "LongWindowSet" if args.long else "DeviceWindowSet", "window": W, "span_rows": N, "series": S, "pairs": K,
           "lags": L, "rows": args.rows, "nan": args.nan, "rounds": args.rounds, "pair_products": products,
           "lags_verified": checked, "verified": True, "unit": "us per call (HIP events)"}
    for k in calls:
        v = sorted(single[k])
        res[k] = {"single_p50": round(statistics.median(v), 2), "single_p10": round(v[len(v) // 10], 2),
                  "single_p90": round(v[len(v) * 9 // 10], 2), "back_to_back_mean": round(statistics.mean(batch[k]), 2),
                  "back_to_back_min": round(min(batch[k]), 2)}
    for m in ("single_p50", "back_to_back_mean"):
        for k in calls:
            res[f"giga_pair_products_per_s_{k}_{m}"] = round(products[k] / res[k][m] / 1e3, 1)
        res[f"xcorr_rate_over_autocorr_rate_{m}"] = round(
            res[f"giga_pair_products_per_s_export_xcorr_{m}"] / res[f"giga_pair_products_per_s_export_autocorr_{m}"], 3)
    line = json.dumps(res)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
