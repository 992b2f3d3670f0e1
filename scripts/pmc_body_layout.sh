#!/bin/bash
# Address-path PMC passes over the two sweeps and the stream-ceiling copy of ONE bench.py run each: how busy the texture
# addresser (TA) and the vector L1 (TCP) are, and what the waves wait for.  Counters only, no tracing flag beside them.
# Usage (GPU box): scripts/pmc_body_layout.sh <tag> [tree, default .]  -> $PMC_OUT/pmclayout_<tag>/summary.txt
# (PMC_OUT: where the passes are kept, default ./pmc_out)
# A pass that ends on a signal or a time limit ends the script: nothing more is started on the GPU after it.
TAG=${1:-head}
TREE=${2:-.}
export TMPDIR=/tmp
OUT=${PMC_OUT:-$PWD/pmc_out}/pmclayout_$TAG
rm -rf "$OUT"; mkdir -p "$OUT"
BENCH="$(cd "$TREE" && pwd)/bench.py"
rocprofv3 --list-avail 2>/dev/null | grep -oE "\b(TA|TCP|TD)_[A-Z0-9_]+" | sort -u > "$OUT/avail_ta_tcp.txt"
cd /tmp
i=0
# (the TA takes two counters per pass: a third ends rocprofv3 with "exceeds the capabilities of the hardware" before the
# program starts, and the profiler then sits until its time limit -- watched for below)
for SET in "TA_TA_BUSY_sum TA_ADDR_STALLED_BY_TC_CYCLES_sum TCP_PENDING_STALL_CYCLES_sum TCP_TCP_TA_DATA_STALL_CYCLES_sum TCP_TCP_TA_ADDR_STALL_CYCLES_sum SQ_WAVE_CYCLES SQ_WAIT_INST_ANY GRBM_GUI_ACTIVE" \
           "TA_DATA_STALLED_BY_TC_CYCLES_sum TA_FLAT_READ_WAVEFRONTS_sum TCP_GATE_EN1_sum TCP_TOTAL_ACCESSES_sum TCP_TCC_READ_REQ_sum SQ_BUSY_CYCLES SQ_ACTIVE_INST_VMEM SQ_WAIT_ANY" \
           "TA_TA_BUSY_sum TCP_PENDING_STALL_CYCLES_sum GRBM_GUI_ACTIVE"; do
  i=$((i+1))
  if [ $i -eq 3 ] && [ -z "$REJECTED" ]; then continue; fi  # (the single-counter pass only stands in for a rejected one)
  timeout -k 10 240 rocprofv3 --pmc $SET --output-format csv -T --kernel-include-regex "k_constraint|k_body|k_copy" -d "$OUT/p$i" -- python3 "$BENCH" --full --steps 1 --warmup 0 --no-cpu-baseline --relaxed-steps 0 > "$OUT/p$i.json" 2> "$OUT/p$i.err" &
  pid=$!
  for t in $(seq 12); do  # a rejected counter set shows in the first seconds: end the profiler instead of waiting it out
    sleep 2
    if grep -q "Could not construct profile cfg" "$OUT/p$i.err" 2>/dev/null; then kill -TERM $pid 2>/dev/null; break; fi  # (timeout passes the signal on, and kills after 10 s)
  done
  wait $pid
  rc=$?
  if grep -q "Could not construct profile cfg" "$OUT/p$i.err"; then echo "pass $i: the counter set was rejected ($SET)"; REJECTED=1; continue; fi
  # any other failure ends the script: nothing more is started on the GPU after a run that did not end well
  if [ $rc -ne 0 ]; then echo "pass $i ($SET) ended with status $rc: stopping"; tail -5 "$OUT/p$i.err"; exit $rc; fi
  echo "pass $i done: $SET"
done
cd - > /dev/null
python3 - "$OUT" <<'PY' > "$OUT/summary.txt"
import csv, glob, os, sys, statistics
from collections import defaultdict
out = sys.argv[1]
acc = defaultdict(lambda: defaultdict(list))
for f in glob.glob(os.path.join(out, "p*", "**", "*counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].split("(")[0].split("<")[0]
        acc[k][r["Counter_Name"]].append((float(r["Counter_Value"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
print("# mean per EFFECTIVE launch (duration >= half the median of that kernel in that pass); durations under the counters in us")
for k in sorted(acc):
    print("\n## " + k)
    for c in sorted(acc[k]):
        v = acc[k][c]
        med = statistics.median(d for _, d in v)
        e = [(x, d) for x, d in v if d >= 0.5 * med]
        print("%-44s %14.4g   launches %5d  mean duration %.1f us" % (c, sum(x for x, _ in e) / len(e), len(e), sum(d for _, d in e) / len(e) / 1e3))
PY
cat "$OUT/summary.txt"
