"""The auto gridder (Options(gridder="auto")) beside the default
(MFMA) and the ordered gridder, in one GPU call through the device entries
with HIP-event timing: after a warm-up of each leg, REPS rounds of the legs
interleaved on the same resident batch.  Modes are chosen by idg_amd.Options,
not by the environment (the one exception: IDG_AUTO_SLICES, the workgroups per
selected subgrid of the ordered pass, which is no option).  Three batches:

  none_selected  BASELINE configs[1]: 24,500 subgrids, T x C = 2,048 -- auto
                 against default.  Margin: the launches auto adds (a 4-byte
                 memset, the classification, the ordered pass that finds an
                 empty queue) x the fixed cost per launch (28 us, DESIGN.md
                 §8 item 2) + the round-to-round spread of the default leg.
  all_selected   BASELINE configs[2] at NR_TIMESLOTS = 4: 4,900 subgrids,
                 T x C = 32,768 -- auto against ordered.  Margin: the same
                 launches + the default gridder on the all-empty batch, a leg
                 of its own.
  sparse         that batch with nr_timesteps cut to 32 on all but every 50th
                 subgrid (98 of 4,900 selected) -- default, ordered, auto with
                 1 slice per subgrid and with finer slicings.  The ordered
                 pass's share of auto's time is 1 - (auto with a threshold
                 nothing exceeds) / auto.

and, for six sampled subgrids per batch, each leg's reference-metric distance
to the oracle.  Times are per launch sequence (median, min and all rounds).

    python tools/debug/auto_rate.py [--out profiles/auto/rate.json] [--reps 7]
                                    [--batches none_selected,all_selected,sparse]
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

LAUNCH_MS = 0.028       # fixed cost per launch, DESIGN.md §8 item 2
AUTO_EXTRA_LAUNCHES = 3  # memset of the count, classification, ordered pass
CONFIGS1 = (50, 20, 128, 16, 1024, 32)
CONFIGS2_TS4 = (50, 4, 128, 256, 1024, 32)
NEVER = 2 ** 32 - 1     # a threshold no product of this tool exceeds


def legs_for(idg, batch):
    """name -> (Options, IDG_AUTO_SLICES or None, metadata key)."""
    O = idg.Options
    if batch == "none_selected":
        return {"default": (O(gridder="default"), None, "md"),
                "auto": (O(gridder="auto"), None, "md")}
    if batch == "all_selected":
        return {"ordered": (O(gridder="ordered"), None, "md"),
                "auto": (O(gridder="auto"), None, "md"),
                "default_on_empty": (O(gridder="default"), None, "empty")}
    return {"default": (O(gridder="default"), None, "md"),
            "ordered": (O(gridder="ordered"), None, "md"),
            "auto_1_slice": (O(gridder="auto"), "1", "md"),
            "auto_2_slices": (O(gridder="auto"), "2", "md"),
            "auto_4_slices": (O(gridder="auto"), "4", "md"),
            "auto_nothing_selected": (O(gridder="auto", auto_threshold=NEVER),
                                      "2", "md")}


def run_batch(idg, o, batch, reps):
    import torch
    st, ts, T, C, G, S = CONFIGS1 if batch == "none_selected" else CONFIGS2_TS4
    a = idg.generate(st, ts, T, C, G, S, nthreads=16)
    ns = idg.nr_subgrids_for(st, ts)
    md = a["metadata"].copy()
    if batch == "sparse":
        cut = np.arange(ns) % 50 != 0
        md["nr_timesteps"][cut] = 32
    empty = md.copy()
    empty["nr_timesteps"] = 0
    params = (ns, G, S, idg.IMAGE_SIZE, 0.0, C, st)
    dev = {k: torch.from_numpy(a[k]).cuda() for k in
           ("uvw", "wavenumbers", "visibilities", "spheroidal", "aterms")}
    mds = {k: torch.from_numpy(v.view(np.int32).reshape(-1, 9).copy()).cuda()
           for k, v in (("md", md), ("empty", empty))}
    legs = legs_for(idg, batch)
    selected = idg.auto_selected(md, C, idg.Options(gridder="auto"))
    out = {m: torch.empty((ns, 4, S, S, 2), dtype=torch.float32,
                          device="cuda") for m in legs}

    def launch(leg):
        opt, slices, key = legs[leg]
        if slices is None:
            os.environ.pop("IDG_AUTO_SLICES", None)
        else:
            os.environ["IDG_AUTO_SLICES"] = slices
        idg.gridder_launch(*params, dev["uvw"], dev["wavenumbers"],
                           dev["visibilities"], dev["spheroidal"],
                           dev["aterms"], mds[key], out[leg], options=opt)

    for leg in legs:   # warm-up: code objects, workspaces, clocks
        launch(leg)
    torch.cuda.synchronize()
    ms = {m: [] for m in legs}
    for _ in range(reps):
        for leg in legs:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(leg)
            e1.record()
            e1.synchronize()
            ms[leg].append(e0.elapsed_time(e1))
    os.environ.pop("IDG_AUTO_SLICES", None)

    # six sampled subgrids against the oracle; on the sparse batch half of
    # them selected ones
    if batch == "sparse":
        samples = sorted({0, 1, 50 * (ns // 100), ns // 2 + 3,
                          50 * ((ns - 1) // 50), ns - 1})
    else:
        samples = sorted({0, 1, ns // 3, ns // 2 + 3, ns - 2, ns - 1})
    one = (1, G, S, idg.IMAGE_SIZE, 0.0, C, st)
    checked = [m for m in legs if legs[m][2] == "md"]
    dist = {m: [] for m in checked}
    for s in samples:
        md0 = md[s:s + 1].copy()
        md0["time_offset"] = 0
        md0["baseline_offset"] = 0
        go = np.zeros((1, 4, S, S, 2), np.float32)
        o.gridder(*one, np.ascontiguousarray(a["uvw"][s]), a["wavenumbers"],
                  np.ascontiguousarray(a["visibilities"][s]),
                  a["spheroidal"], a["aterms"], md0, go)
        for m in checked:
            dist[m].append(float(o.check_error(
                out[m][s:s + 1].cpu().numpy(), go)[0]))
    med = {m: float(np.median(ms[m])) for m in legs}
    spread = {m: float(max(ms[m]) - min(ms[m])) for m in legs}
    res = {
        "shape": dict(nr_stations=st, nr_timeslots=ts, nr_timesteps=T,
                      nr_channels=C, grid_size=G, subgrid_size=S,
                      nr_subgrids=ns),
        "selected_subgrids": int(selected.sum()),
        "gridder_ms": {m: {"median": med[m], "min": float(min(ms[m])),
                           "spread": spread[m],
                           "all": [round(x, 4) for x in ms[m]]}
                       for m in legs},
        "sampled_subgrids": samples,
        "sampled_selected": [int(selected[s]) for s in samples],
        "distance_to_oracle": dist,
        "distance_to_oracle_max": {m: max(dist[m]) for m in checked},
    }
    launches = AUTO_EXTRA_LAUNCHES * LAUNCH_MS
    if batch == "none_selected":
        res["auto_minus_default_ms"] = med["auto"] - med["default"]
        res["margin_ms"] = launches + spread["default"]
        res["within_margin"] = res["auto_minus_default_ms"] <= res["margin_ms"]
    elif batch == "all_selected":
        res["auto_minus_ordered_ms"] = med["auto"] - med["ordered"]
        res["margin_ms"] = launches + med["default_on_empty"]
        res["within_margin"] = res["auto_minus_ordered_ms"] <= res["margin_ms"]
    else:
        autos = {m: med[m] for m in legs if m.startswith("auto_")
                 and m != "auto_nothing_selected"}
        kept = min(autos, key=autos.get)
        res["fastest_slicing"] = kept
        res["auto_over_ordered"] = {m: autos[m] / med["ordered"]
                                    for m in autos}
        res["auto_over_default"] = {m: autos[m] / med["default"]
                                    for m in autos}
        res["ordered_pass_share_of_auto"] = {
            m: 1.0 - med["auto_nothing_selected"] / autos[m] for m in autos}
        res["auto_faster_than_ordered"] = autos[kept] < med["ordered"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "auto",
                                                  "rate.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="none_selected,all_selected,sparse")
    args = ap.parse_args()
    import torch
    import idg_amd
    import oracle
    assert torch.cuda.is_available(), "needs a HIP device"
    res = {"device": idg_amd.device_name(), "reps": args.reps,
           "launch_ms": LAUNCH_MS, "auto_extra_launches": AUTO_EXTRA_LAUNCHES,
           "auto_threshold": idg_amd.api.AUTO_THRESHOLD}
    for name in args.batches.split(","):
        r = res[name] = run_batch(idg_amd, oracle.Oracle(), name, args.reps)
        print(name, {m: round(v["median"], 3)
                     for m, v in r["gridder_ms"].items()},
              {k: v for k, v in r.items()
               if k in ("margin_ms", "within_margin", "fastest_slicing",
                        "auto_faster_than_ordered", "auto_minus_default_ms",
                        "auto_minus_ordered_ms")},
              {m: "%.2e" % v for m, v in r["distance_to_oracle_max"].items()},
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
