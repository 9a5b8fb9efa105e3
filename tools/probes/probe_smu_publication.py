"""When does the SMU firmware publish a new gpu_metrics table?

Reads the amdgpu ``gpu_metrics`` blob of GPU 0 back to back for ``--seconds`` (no
tracking, every read an SMU round trip) and records, for every publication (the v1.8
table's firmware timestamp moved): the firmware-timestamp delta (10 ns units) and the
host time at which the read that saw it started. From these:

  fw_interval_us     the publication period as the firmware stamps it (it moves in ~1 ms
                     steps: fw_interval_ms_histogram)
  host_interval_us   the same between the detecting reads (adds up to one read of latency)
  predict_error_us   detection time minus (previous detection + P), P the running period
                     estimate SmuTableTracker keeps (host intervals, P += (interval - P) / 8):
                     what the tracker's guard has to cover on either side

The guard and hard bound of csrc/sources.h (kSmuGuardNs, kSmuHardNs) come from this
output (profiles/smu_track/publication_intervals.json).

    python tools/probes/probe_smu_publication.py --seconds 12 --out FILE.json
    python tools/probes/probe_smu_publication.py --reanalyse FILE.json   # the summaries again, from a recording
"""

from __future__ import annotations

import argparse
import json
import os
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

FW_TS_OFFSET = 288  # csrc/sources.cpp kV18Interconnect.fw_ts


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q / 100.0 * len(s)))] if s else None


def summary(v):
    return {"n": len(v), "min": round(min(v), 1), "p1": round(pct(v, 1), 1), "p50": round(pct(v, 50), 1),
            "p99": round(pct(v, 99), 1), "max": round(max(v), 1)} if v else {"n": 0}


def analyse(fw_us, host_us):
    err = []
    p = None
    for h in host_us:
        if p is not None:
            err.append(h - p)
        p = h if p is None else p + (h - p) / 8
    ticks = {}
    for x in fw_us:
        ticks[str(round(x / 100.0) / 10.0)] = ticks.get(str(round(x / 100.0) / 10.0), 0) + 1
    return {"fw_interval_us": summary(fw_us), "host_interval_us": summary(host_us), "predict_error_us": summary(err),
            "fw_interval_ms_histogram": dict(sorted(ticks.items()))}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reanalyse", default=None, metavar="FILE")
    args = ap.parse_args()
    if args.reanalyse:
        with open(args.reanalyse) as f:
            out = json.load(f)
        out.update(analyse(out["fw_interval_us_all"], out["host_interval_us_all"]))
        with open(args.out or args.reanalyse, "w") as f:
            json.dump(out, f)
        print(json.dumps({k: v for k, v in out.items() if not k.endswith("_all")}))
        return 0
    from rocmdash.runtime import native

    nat = native.load()
    gpus = nat.amdsmi_enumerate()
    if not gpus:
        print(json.dumps({"error": "no AMD GPU"}))
        return 1
    bdf = int(gpus[0]["bdf"])
    path = "/sys/bus/pci/devices/%04x:%02x:%02x.%x/gpu_metrics" % (bdf >> 32, (bdf >> 8) & 0xFF, (bdf >> 3) & 0x1F, bdf & 7)
    fd = os.open(path, os.O_RDONLY)
    head = os.pread(fd, 4096, 0)
    size, fmt, content = struct.unpack_from("<HBB", head, 0)
    if fmt != 1 or content != 8 or size < FW_TS_OFFSET + 8:
        print(json.dumps({"error": f"not a v1.8 table: v{fmt}.{content} {size} B"}))
        return 1
    reads = 0
    read_us = []
    fw, host = [], []
    last = struct.unpack_from("<Q", head, FW_TS_OFFSET)[0]
    end = time.perf_counter() + args.seconds
    while True:
        t0 = time.perf_counter_ns()
        b = os.pread(fd, size, 0)
        t1 = time.perf_counter_ns()
        reads += 1
        if reads % 16 == 0:
            read_us.append((t1 - t0) / 1e3)
        ts = struct.unpack_from("<Q", b, FW_TS_OFFSET)[0]
        if ts != last:
            fw.append(ts - last)
            host.append(t0)
            last = ts
        if t1 * 1e-9 >= end:
            break
    os.close(fd)
    fw_us = [d / 100.0 for d in fw[1:]]  # 10 ns units; the first delta started before the loop
    host_us = [(b - a) / 1e3 for a, b in zip(host, host[1:])]
    out = {"table": f"v{fmt}.{content} {size} B", "seconds": args.seconds, "reads": reads,
           "reads_per_s": round(reads / args.seconds, 1), "publications": len(fw),
           "publications_per_s": round(len(fw) / args.seconds, 2), "read_us": summary(read_us),
           "fw_interval_us_all": [round(x, 2) for x in fw_us], "host_interval_us_all": [round(x, 1) for x in host_us]}
    out.update(analyse(fw_us, host_us))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)
    print(json.dumps({k: v for k, v in out.items() if not k.endswith("_all")}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
