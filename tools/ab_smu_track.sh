#!/bin/bash
# A/B on one MI355X box of the SMU table publication tracking and of the stats launch at
# the row mix it brings, alternating, the default (free-running) N = 1 bench:
#   track      the default: the table read only around publications, small_k 2
#   notrack    ROCMDASH_SMU_TABLE_TRACK=0: every amd-smi row reads the table
#   smallk8    ROCMDASH_SMALL_K_ROWS=8: 512 threads up to 8 entering rows
# Usage: bash tools/ab_smu_track.sh [OUT_DIR] [ROUNDS] [STEPS]
# (against another built tree: tools/ab_tree_bench.sh; the publication intervals the
# tracker's guard comes from: tools/probes/probe_smu_publication.py)
set -u -o pipefail
cd "$(dirname "$0")/.."
O=${1:-build/smu_track}; ROUNDS=${2:-5}; STEPS=${3:-4000}
mkdir -p "$O"
python3 -m rocmdash._build --check || exit 3
for i in $(seq 1 "$ROUNDS"); do
  for arm in track notrack smallk8; do
    case $arm in
      track) e=(ROCMDASH_SMU_TABLE_TRACK=1) ;;
      notrack) e=(ROCMDASH_SMU_TABLE_TRACK=0) ;;
      smallk8) e=(ROCMDASH_SMALL_K_ROWS=8) ;;
    esac
    env "${e[@]}" timeout -k 10 240 python3 bench.py --steps "$STEPS" --json-out "$O/${arm}_$i.json" \
      > "$O/${arm}_$i.log" 2>&1 || { echo "FAILED $arm round $i"; tail -5 "$O/${arm}_$i.log"; exit 1; }
    python3 - "$O/${arm}_$i.json" "$arm" "$i" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(sys.argv[2], sys.argv[3], d["value"], d["fresh_per_s_by_source"], d.get("smu_table_reads_per_s"),
      d.get("smi_table_refreshes_per_s"), d["sampler_p50_us"], d["sampler_mean_us"], d["p50_refresh_ms"], d["p90_refresh_ms"],
      d["p50_breakdown_ms"])
PY
  done
done
