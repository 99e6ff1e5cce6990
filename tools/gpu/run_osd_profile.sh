#!/bin/bash
# BP + OSD evidence (DESIGN.md sections 7.6, 7.7): a rocprofv3 kernel-trace --stats pass of one
# qec_monte_carlo call with QEC_OPT_OSD on per p (a run of its own each), the on / off rates and the
# outcome table (tools/gpu/osd_profile.py), reduced into OUT/osd_p61.json.  Stops at the first failing step.
#   bash tools/gpu/run_osd_profile.sh OUTDIR [p ...]
# ORDER=L in the environment sets QEC_OPT_OSD_ORDER for every step (default 0; written into the JSON);
# ORDER="0 10 60" takes the traces once per order, and with a non-zero order among them the rates and
# the table are the sweep's (cs_rates, cs_table) and the result is OUT/osd_cs_p61.json.
set -o pipefail
R="$(cd "$(dirname "$0")/../.." && pwd)"
OUT=${1:?output directory}; shift
PS=${@:-0.05 0.1}
ORDER=${ORDER:-0}
mkdir -p "$OUT"
OUT="$(cd "$OUT" && pwd)"
export TMPDIR=/tmp
cd /tmp
for L in $ORDER; do
  for P in $PS; do
    D="$OUT/trace_o${L}_p$P"; mkdir -p "$D"
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$D/trace" -o run -- \
        python3 "$R/tools/gpu/osd_profile.py" run --p $P --order $L > "$D/run.out" 2> "$D/run.err" || { tail -5 "$D/run.err"; exit 1; }
    tail -1 "$D/run.out" | cut -c1-300
  done
done
cd "$R"
if [ "$ORDER" = "0" ]; then
  timeout -k 10 300 python3 tools/gpu/osd_profile.py rates --out "$OUT/rates.json" > "$OUT/rates.txt" 2>&1 || { tail -5 "$OUT/rates.txt"; exit 1; }
  timeout -k 10 300 python3 tools/gpu/osd_profile.py table --out "$OUT/table.json" > "$OUT/table.txt" 2>&1 || { tail -5 "$OUT/table.txt"; exit 1; }
  timeout -k 10 120 python3 tools/gpu/osd_profile.py reduce --dir "$OUT" --out "$OUT/osd_p61.json" || exit 1
else
  timeout -k 10 400 python3 tools/gpu/osd_profile.py cs_rates --out "$OUT/cs_rates.json" > "$OUT/cs_rates.txt" 2>&1 || { tail -5 "$OUT/cs_rates.txt"; exit 1; }
  timeout -k 10 300 python3 tools/gpu/osd_profile.py cs_table --out "$OUT/cs_table.json" > "$OUT/cs_table.txt" 2>&1 || { tail -5 "$OUT/cs_table.txt"; exit 1; }
  timeout -k 10 120 python3 tools/gpu/osd_profile.py reduce --dir "$OUT" --out "$OUT/osd_cs_p61.json" || exit 1
fi
