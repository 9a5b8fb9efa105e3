"""HIP-event time of DeviceWindowSet.export_buckets beside export_sorted's - the existing
kernel of the same launch shape (one launch over every series' resident sorted window) -
and of bucket_blocks over N ranks' gathered blocks.

    python tools/bench_window_buckets.py [--window 4096 --series 16 --buckets 16 --ranks 8] [--json-out FILE]

Each figure is measured two ways, alternating the kernels round by round: one call between
two events (median over the rounds; on an idle GPU that span includes the launch's own
start-up), and 100 calls back to back between two events, divided by 100.
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

    from rocmdash.ops.window_buckets import default_bounds
    from rocmdash.models.schema import series_names
    from rocmdash.runtime import native

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--series", type=int, default=16)
    ap.add_argument("--buckets", type=int, default=16)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_buckets: no GPU")
    nat = native.load()
    dev = torch.device("cuda", 0)
    W, S, B, N = args.window, args.series, args.buckets, args.ranks
    nat.set_pinned_host_rings(True)
    ring = nat.SeriesRing(S, 4 * W)
    dws = nat.DeviceWindowSet(W, 0)
    dws.add_ring(ring)
    rng = np.random.default_rng(0)
    x = rng.normal(50.0, 20.0, (W + 3, S)).astype(np.float32)  # telemetry-like: spread over the default axes
    ring.push_many(x, np.arange(1, W + 4, dtype=np.uint64))
    names = (series_names() * (S // len(series_names()) + 1))[:S]
    bounds = torch.from_numpy(default_bounds(names, buckets=B)).to(dev)
    out = torch.empty((S, 8), device=dev)
    sorted_dst = torch.empty((S, W + 1), device=dev)
    bucket_dst = torch.empty((S, B + 1), device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    dws.refresh(out.data_ptr(), stream, 50.0, 90.0, 99.0)
    torch.cuda.synchronize()
    blocks = torch.empty((N, S, W + 1), device=dev)  # every rank this window's export block
    per_rank = torch.empty((N, S, B + 1), device=dev)
    node = torch.empty((S, B + 1), device=dev)

    calls = {
        "export_sorted": lambda: dws.export_sorted(sorted_dst.data_ptr(), stream),
        "export_buckets": lambda: dws.export_buckets(bounds.data_ptr(), B, bucket_dst.data_ptr(), stream),
        f"bucket_blocks_n{N}": lambda: nat.bucket_blocks(blocks.data_ptr(), N, S, W, bounds.data_ptr(), B,
                                                         per_rank.data_ptr(), node.data_ptr(), stream),
    }
    dws.export_sorted(sorted_dst.data_ptr(), stream)
    torch.cuda.synchronize()
    blocks.copy_(sorted_dst.unsqueeze(0).expand(N, S, W + 1))
    for f in calls.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    assert float(bucket_dst[:, -1].min()) == W and torch.equal(node, per_rank.sum(dim=0))

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
    res = {"window": W, "series": S, "buckets": B, "ranks": N, "rounds": args.rounds, "unit": "us per call (HIP events)"}
    for k in calls:
        v = sorted(single[k])
        res[k] = {"single_p50": round(statistics.median(v), 2), "single_p10": round(v[len(v) // 10], 2),
                  "single_p90": round(v[len(v) * 9 // 10], 2), "back_to_back_mean": round(statistics.mean(batch[k]), 2),
                  "back_to_back_min": round(min(batch[k]), 2)}
    res["buckets_over_sorted"] = {m: round(res["export_buckets"][m] / res["export_sorted"][m], 2)
                                  for m in ("single_p50", "back_to_back_mean")}
    line = json.dumps(res)
    print(line)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
