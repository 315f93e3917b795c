"""The ordered gridder (IDG_GRIDDER_IMPL=ordered) beside the sequential and
the default (MFMA) gridder, in one GPU call through the device entries with
HIP-event timing: after a warm-up of each, REPS rounds of sequential ->
ordered -> mfma launches on the same resident batch, at

  configs1   BASELINE configs[1]: 24,500 subgrids, C = 16
  configs2   BASELINE configs[2] at NR_TIMESLOTS = 4 (4,900 subgrids, C = 256;
             the shape of bench.py's sequential.configs2)

and, for six sampled subgrids per shape, the reference-metric distance of
each mode's output to the oracle (bit-exact to the reference's CPU output).
Times are per launch (median and min of the rounds); the throughput figure of
record stays bench.py's.

    python tools/debug/ordered_rate.py [--out profiles/ordered/rate.json]
                                       [--reps 5] [--shapes configs1,configs2]
--modes ordered --no-distance --out - : the launches alone, for a profiler
(tools/probes/pmc_ordered.sh).
DESIGN.md §3.5.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-idg-bench_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

SHAPES = {
    # (stations, timeslots, T, C, G, S)
    "configs1": (50, 20, 128, 16, 1024, 32),
    "configs2": (50, 4, 128, 256, 1024, 32),
}
MODES = ("sequential", "ordered", "mfma")


def run_shape(idg, o, name, reps, modes=MODES, distance=True):
    import torch
    st, ts, T, C, G, S = SHAPES[name]
    a = idg.generate(st, ts, T, C, G, S, nthreads=16)
    ns = idg.nr_subgrids_for(st, ts)
    params = (ns, G, S, idg.IMAGE_SIZE, 0.0, C, st)
    dev = {k: torch.from_numpy(a[k]).cuda() for k in
           ("uvw", "wavenumbers", "visibilities", "spheroidal", "aterms")}
    dev["metadata"] = torch.from_numpy(
        a["metadata"].view(np.int32).reshape(-1, 9).copy()).cuda()
    out = {m: torch.empty((ns, 4, S, S, 2), dtype=torch.float32,
                          device="cuda") for m in modes}

    def launch(mode):
        os.environ["IDG_GRIDDER_IMPL"] = mode
        idg.gridder_launch(*params, dev["uvw"], dev["wavenumbers"],
                           dev["visibilities"], dev["spheroidal"],
                           dev["aterms"], dev["metadata"], out[mode])

    kernels = {}
    for mode in modes:  # warm-up: code objects, workspaces, clocks
        launch(mode)
        kernels[mode] = idg.kernel_name("gridder", S, C)
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    for _ in range(reps):
        for mode in modes:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(mode)
            e1.record()
            e1.synchronize()
            ms[mode].append(e0.elapsed_time(e1))
    os.environ.pop("IDG_GRIDDER_IMPL", None)
    if not distance:
        return {"kernels": kernels, "gridder_ms": ms}

    samples = sorted({0, 1, ns // 3, ns // 2 + 3, ns - 2, ns - 1})
    one = (1, G, S, idg.IMAGE_SIZE, 0.0, C, st)
    dist = {m: [] for m in modes}
    for s in samples:
        md0 = a["metadata"][s:s + 1].copy()
        md0["time_offset"] = 0
        md0["baseline_offset"] = 0
        go = np.zeros((1, 4, S, S, 2), np.float32)
        o.gridder(*one, np.ascontiguousarray(a["uvw"][s]), a["wavenumbers"],
                  np.ascontiguousarray(a["visibilities"][s]),
                  a["spheroidal"], a["aterms"], md0, go)
        for m in modes:
            dist[m].append(float(o.check_error(
                out[m][s:s + 1].cpu().numpy(), go)[0]))
    med = {m: float(np.median(ms[m])) for m in modes}
    return {
        "shape": dict(nr_stations=st, nr_timeslots=ts, nr_timesteps=T,
                      nr_channels=C, grid_size=G, subgrid_size=S,
                      nr_subgrids=ns),
        "kernels": kernels,
        "gridder_ms": {m: {"median": med[m], "min": float(min(ms[m])),
                           "all": [round(x, 4) for x in ms[m]]}
                       for m in modes},
        **{f"ordered_over_{m}": med["ordered"] / med[m]
           for m in modes if m != "ordered" and "ordered" in med},
        "sampled_subgrids": samples,
        "distance_to_oracle": dist,
        "distance_to_oracle_max": {m: max(dist[m]) for m in modes},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ordered",
                                                  "rate.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="configs1,configs2")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--no-distance", action="store_true")
    args = ap.parse_args()
    modes = tuple(args.modes.split(","))
    import torch
    import idg_amd
    import oracle
    assert torch.cuda.is_available(), "needs a HIP device"
    res = {"device": idg_amd.device_name(), "reps": args.reps,
           "modes": list(modes)}
    for name in args.shapes.split(","):
        res[name] = run_shape(idg_amd, oracle.Oracle(), name, args.reps,
                              modes, not args.no_distance)
        r = res[name]
        if args.no_distance:
            print(name, r, flush=True)
            continue
        print(name, {m: round(r["gridder_ms"][m]["median"], 3) for m in modes},
              {k: round(v, 3) for k, v in r.items() if "_over_" in k},
              {m: "%.2e" % r["distance_to_oracle_max"][m] for m in modes},
              flush=True)
        torch.cuda.empty_cache()
    if args.out == "-":
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
