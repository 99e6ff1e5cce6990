#!/bin/bash
# BP + OSD-0 evidence: a rocprofv3 kernel-trace --stats pass of one qec_monte_carlo
# call with QEC_OPT_OSD on per p (a run of its own each), the on / off rates and the outcome table
# (tools/gpu/osd_profile.py), reduced into OUT/osd_p61.json.  Stops at the first failing step.
#   bash tools/gpu/run_osd_profile.sh OUTDIR [p ...]
set -o pipefail
R="$(cd "$(dirname "$0")/../.." && pwd)"
OUT=${1:?output directory}; shift
PS=${@:-0.05 0.1}
mkdir -p "$OUT"
OUT="$(cd "$OUT" && pwd)"
export TMPDIR=/tmp
cd /tmp
for P in $PS; do
  D="$OUT/trace_p$P"; mkdir -p "$D"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$D/trace" -o run -- \
      python3 "$R/tools/gpu/osd_profile.py" run --p $P > "$D/run.out" 2> "$D/run.err" || { tail -5 "$D/run.err"; exit 1; }
  tail -1 "$D/run.out" | cut -c1-300
done
cd "$R"
timeout -k 10 300 python3 tools/gpu/osd_profile.py rates --out "$OUT/rates.json" > "$OUT/rates.txt" 2>&1 || { tail -5 "$OUT/rates.txt"; exit 1; }
timeout -k 10 300 python3 tools/gpu/osd_profile.py table --out "$OUT/table.json" > "$OUT/table.txt" 2>&1 || { tail -5 "$OUT/table.txt"; exit 1; }
timeout -k 10 120 python3 tools/gpu/osd_profile.py reduce --dir "$OUT" --out "$OUT/osd_p61.json" || exit 1
