#!/bin/bash
# A/B of library variants on the pipeline steps (FFT, adder, splitter ms).
# The bench lines go to $OUT (default: a fresh temporary directory).
set -o pipefail
cd "$GRAFT_REPO_ROOT"
out=${OUT:-$(mktemp -d)}
mkdir -p "$out"
for rep in 1 2; do
for lib in "$@"; do
  n=$(basename $lib .so)
  IDG_MI355X_LIB=$PWD/$lib timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 5 ${BENCH_ARGS:-} > "$out/$n.json" 2> "$out/$n.err" || { tail -5 "$out/$n.err"; exit 1; }
  python -c "
import json; d=json.load(open('$out/$n.json')); p=d['pipeline']; print('$n', p['fft_ms'], p['adder_ms'], p['splitter_ms'], p['ifft_ms'], p.get('splitter_fft_ms'), p.get('gridder_fft_ms'), p.get('gridder_then_fft_ms'), p.get('full_cycle_mvis_s'), p.get('full_cycle_fused_mvis_s'))"
done
done
