"""HIP-event time of export_periods (the autocorrelation's lags 0 .. L per trend column of the
newest SPAN rows) beside export_autocorr over the same ring, span and lags in the same process,
and the host's share of a collection: the D2H copy of the sums and ``slot_periods`` over them.

    python tools/bench_window_periods.py [--window 4096 --series 16 --columns 8 --lags 64] [--json-out FILE]
    python tools/bench_window_periods.py --long --window 65536 --series 12 --columns 64 --lags 255
    python tools/bench_window_periods.py --long --window 1048576 --span 1048576 --series 12 --columns 16 --lags 255 --splits 1,8

The set's result is verified first, every word against the reference (for N x L above 2^27 on a
sample of the lags, through the one-lag sums of every slot). ``--splits``: also time the one-shot
entry over a copy of the same rows with these splits forced (1 = a workgroup owns its slot; 0 = the
plan's own choice through that entry), each verified bit for bit against the set's result. Then one
call between two events, warm, the median over the rounds, and 20 calls back to back between two
events divided by 20, the calls alternating. ``--rows`` and ``--nan`` as bench_window_autocorr.py.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    import torch

    from rocmdash.ops.window_autocorr import quantise
    from rocmdash.ops.window_periods import check_periods, periods_geometry, slot_periods, window_periods_reference
    from rocmdash.runtime import native

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--series", type=int, default=16)
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--lags", type=int, default=64)
    ap.add_argument("--span", type=int, default=None)
    ap.add_argument("--long", action="store_true", help="a LongWindowSet (windows of 2^10 .. 2^26 rows)")
    ap.add_argument("--rows", choices=["telemetry", "independent"], default="telemetry")
    ap.add_argument("--nan", type=float, default=0.0, help="share of NaN samples")
    ap.add_argument("--splits", default="", help="comma-separated splits to force through the one-shot entry")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_periods: no GPU")
    nat = native.load()
    dev = torch.device("cuda", 0)
    W, S = args.window, args.series
    P, L, span = check_periods(args.columns, args.lags, args.span, W)
    N = min(W, span)
    splits = [int(s) for s in args.splits.split(",") if s.strip()]
    nat.set_pinned_host_rings(True)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((S, 8), device=dev)
    dst = torch.full((S, P + 1, L + 1, 4), -1, dtype=torch.int64, device=dev)
    whole = torch.full((S, L + 1, 4), -1, dtype=torch.int64, device=dev)
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

    total = W + 1000  # a full window in a wrapped device ring; the oldest and the newest slot are partial
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

    calls = {"export_periods": lambda: ws.export_periods(span, P, sd.data_ptr(), L, dst.data_ptr(), stream),
             "export_autocorr": lambda: ws.export_autocorr(span, sd.data_ptr(), L, whole.data_ptr(), stream)}
    newest = block[np.arange(t - N, t) % len(block)]  # rows [t - N, t) of the stream
    one_shot = {}
    if splits:  # the same rows in a ring of W rows described by value
        mem = torch.empty((W, S), dtype=torch.float32, device=dev)
        win = block[np.arange(t - W, t) % len(block)]
        mem[torch.arange(t - W, t, device=dev, dtype=torch.int64) % W] = torch.from_numpy(win).to(dev)
        for sp in splits:
            d = torch.full((S, P + 1, L + 1, 4), -1, dtype=torch.int64, device=dev)
            one_shot[sp] = d
            calls[f"periods_ring_split_{sp}"] = (lambda sp=sp, d=d: nat.periods_ring(
                mem.data_ptr(), S, S, W, t, W, span, P, sd.data_ptr(), L, d.data_ptr(), sp, stream))
    for f in calls.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    _, ranges = periods_geometry(t, N, P, span)
    if N * L <= 1 << 27:
        assert np.array_equal(got, window_periods_reference(newest, scale, t, W, P, L, span)), "export_periods differs from the reference"
        checked = L + 1
    else:  # the same sums, one lag at a time, for a sample of the lags
        q, v = quantise(newest, scale)
        lags = sorted({0, 1, 2, 7, 8, L // 2, L - 1, L})
        for j, (b, e) in enumerate(ranges):
            qs, vs = q[b - (t - N) : e - (t - N)], v[b - (t - N) : e - (t - N)]
            for k in lags:
                m = max(len(qs) - k, 0)
                q0, v0, qk, vk = qs[:m], vs[:m], qs[k : k + m], vs[k : k + m]
                want = np.stack([(v0 * vk).sum(0), (q0 * vk).sum(0), (v0 * qk).sum(0), (q0 * qk).sum(0)], axis=1)
                assert np.array_equal(got[:, j, k], want), f"export_periods differs from the reference at slot {j} lag {k}"
        checked = len(lags)
    for sp, d in one_shot.items():
        assert np.array_equal(d.cpu().numpy(), got), f"periods_ring with split {sp} differs from export_periods"
    assert np.array_equal(got[:, :, 0, 0].sum(axis=1), whole.cpu().numpy()[:, 0, 0]), "the slots' n_0 do not add up to the span's"

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
    d2h, host = [], []
    for _ in range(args.host_rounds):  # the host's share of a collection: the copy, then the periods
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sums = dst.to("cpu", non_blocking=False).numpy()
        t1 = time.perf_counter()
        slot_periods(sums)
        d2h.append((t1 - t0) * 1e3)
        host.append((time.perf_counter() - t1) * 1e3)
    res = {"set": "LongWindowSet" if args.long else "DeviceWindowSet", "window": W, "span_rows": N, "series": S, "columns": P,
           "rows_per_column": span // P, "lags": L, "rows": args.rows, "nan": args.nan, "rounds": args.rounds,
           "output_bytes": int(dst.numel() * 8), "lags_verified": checked, "verified": True, "unit": "us per call (HIP events)"}
    for k in calls:
        v = sorted(single[k])
        res[k] = {"single_p50": round(statistics.median(v), 2), "single_p10": round(v[len(v) // 10], 2),
                  "single_p90": round(v[len(v) * 9 // 10], 2), "back_to_back_mean": round(statistics.mean(batch[k]), 2),
                  "back_to_back_min": round(min(batch[k]), 2)}
    for m in ("single_p50", "back_to_back_mean"):
        res[f"periods_over_autocorr_{m}"] = round(res["export_periods"][m] / res["export_autocorr"][m], 3)
    res["host_ms"] = {"d2h_median": round(statistics.median(d2h), 3), "slot_periods_median": round(statistics.median(host), 1),
                      "rounds": args.host_rounds}
    line = json.dumps(res)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
