#!/bin/bash
# The ordered gridder (IDG_GRIDDER_IMPL=ordered) under rocprofv3: a kernel
# trace, then the SQ instruction-class counters, one run per group (gfx950
# block limits) and no tracing beside the counters.  Every run launches the
# gridder alone on the configs[1] batch (tools/debug/ordered_rate.py --modes
# ordered --no-distance: one warm-up and one more launch).
#   bash tools/probes/pmc_ordered.sh OUTDIR
#   python tools/probes/summarize_ordered.py OUTDIR --out profiles/ordered/pmc.json
# Every GPU step has its own limit; the first failure ends the script.
set -eo pipefail
repo=$(cd "$(dirname "$0")/../.." && pwd)
out=${1:?usage: pmc_ordered.sh OUTDIR}
mkdir -p "$out"
out=$(cd "$out" && pwd)
run="python3 $repo/tools/debug/ordered_rate.py --modes ordered --no-distance --shapes ${SHAPE:-configs1} --reps 1 --out -"
cd "$out"
timeout -k 10 200 rocprofv3 --kernel-trace -d "$out/ktrace" -o run -- $run \
  > "$out/ktrace.out" 2> "$out/ktrace.err" || { echo "kernel trace failed"; exit 1; }
i=0
for grp in "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES" \
           "SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE" \
           "SQ_INSTS_VALU_INT32 SQ_INSTS_VALU_INT64 SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_ADD_F32" \
           "SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_CVT SQ_WAIT_INST_ANY" \
           "SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS SQ_INST_CYCLES_VMEM"; do
  i=$((i+1))
  timeout -s KILL 200 rocprofv3 --pmc $grp -d "$out/p$i" -o run -- $run \
    > /dev/null 2> "$out/p$i.err" || { echo "pass $i failed"; exit 1; }
done
echo done
