"""Per-launch times of Clark CLEAN's kernels from kernel traces
of tools/debug/clark_rate.py, one trace per size: events around a call cannot
separate the cycle kernel, a trace can.

    for s in 1024x256 2048x256 4096x256 2048x2048; do
      rocprofv3 --kernel-trace --output-format csv -d traces/$s -- \\
        python tools/debug/clark_rate.py --reps 1 --out - --sizes $s
    done
    python tools/debug/clark_kernels.py traces [--out profiles/clark/kernels.json]

Such a run of clark_rate.py launches every per-round kernel 20 times: 4 rounds
in the round-by-round pass, 4 in the warm-up window and 4 in the one timed
window of the `clark` form -- the 12 that do work -- and 8 in the two windows
of the `select` form, whose cycle and apply launches have nothing to do.  So
per kernel: calls, the median and maximum over all launches, and
`largest12_median_us`, the median of the twelve longest, which for cycle and
apply are the launches with 1,000 iterations' work (for cycle: divide by
iterations_per_round for the time of one iteration)."""
import argparse
import collections
import csv
import glob
import json
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))


def reduce_trace(directory):
    per = collections.defaultdict(list)
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"),
                       recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                if "kernel_clark" not in name:
                    continue
                short = name[name.index("kernel_clark"):].split("(")[0]
                per[short].append((int(row["End_Timestamp"])
                                   - int(row["Start_Timestamp"])) / 1e3)
    out = {}
    for name, us in sorted(per.items()):
        us = sorted(us)
        out[name] = {"calls": len(us),
                     "median_us": round(float(np.median(us)), 2),
                     "max_us": round(us[-1], 2),
                     "largest12_median_us": round(
                         float(np.median(us[-12:])), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("traces", help="a directory with one trace directory per "
                                   "size, named GxGp")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clark",
                                                  "kernels.json"))
    args = ap.parse_args()
    sizes = sorted(os.listdir(args.traces),
                   key=lambda s: [int(v) for v in s.split("x")][::-1])
    out = {size: reduce_trace(os.path.join(args.traces, size))
           for size in sizes}
    assert all(out.values()), "a trace without clark kernels"
    print(json.dumps({s: {k: v["largest12_median_us"] for k, v in d.items()}
                      for s, d in out.items()}, indent=1))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
