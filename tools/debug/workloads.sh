#!/bin/bash
# Bench line per workload (s64, c256, wterm), with the pipeline steps
# (--full), into $OUT (default: a fresh temporary directory), plus the
# all-VALU A/B reference on wterm.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
out=${OUT:-$(mktemp -d)}
mkdir -p "$out"
for w in ${WORKLOADS:-s64 wterm c256}; do
  steps=5; [ $w = c256 ] && steps=3
  timeout -k 10 400 python bench.py --full --no-cpu-baseline --workload $w --steps $steps > "$out/$w.json" 2> "$out/$w.err" || { tail -5 "$out/$w.err"; exit 1; }
  python -c "
import json; d=json.load(open('$out/$w.json')); k=d['kernels']; print('$w', d['value'], k['gridder']['ms'], k['degridder']['ms'])"
done
IDG_GRIDDER_IMPL=valu IDG_DEGRIDDER_IMPL=valu timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-pipeline --workload wterm --steps 5 > "$out/wterm_valu.json" 2> "$out/wterm_valu.err" || exit 1
python -c "
import json; d=json.load(open('$out/wterm_valu.json')); k=d['kernels']; print('wterm_valu', d['value'], k['gridder']['ms'], k['degridder']['ms'])"
