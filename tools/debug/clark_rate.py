"""Clark CLEAN's time per component, measured, not gated, beside
the Hogbom minor cycle's in the same process: (G, Gp) = (1024, 256),
(2048, 256), (4096, 256) and (2048, 2048) on a residual of 300 sources.

  clark     idg_amd.clark as shipped: one call of ROUNDS rounds of up to
            ITERATIONS components each -- begin, five launches a round, search
            and finish, selection and apply included -- per component taken
  select    the same call with iterations_per_round = 0: every launch of it,
            no component (the histogram, limit and compaction of each round
            and the ends of the call), per component of the `clark` form; what
            is left of `clark` (reported as cycle_plus_apply) is the cycle
            kernel's loop and apply together
  clean     idg_amd.clean for the same number of components, one launch each

HIP events around windows of one call; REPS windows of each form taking turns
after a warm-up window; median, min and max.  Every window starts from the
same residual (restored before the first event, not timed).  The device's
bytes are checked against the host entry's at the first size before anything
is timed.  Candidates and components per round come from a run of one round
per call, not timed.  The cycle kernel alone is not separable with events
around a call: tools/debug/clark_kernels.py reduces kernel traces of this tool
(--reps 1 --out -, one size per trace) to profiles/clark/kernels.json.

    python tools/debug/clark_rate.py [--out profiles/clark/rate.json]
                                     [--reps 7] [--rounds 4]
                                     [--iterations 1000] [--sizes 1024x256,...]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-idg-bench_amd"))

SIZES = [(1024, 256), (2048, 256), (4096, 256), (2048, 2048)]
GAIN = 0.1
SOURCES = 300


def stats(us):
    return {"median": round(float(np.median(us)), 3),
            "min": round(float(min(us)), 3), "max": round(float(max(us)), 3)}


def inputs(G, Gp, seed=1):
    """A smooth PSF (centre 1, sidelobes falling off from 0.1) and a residual
    of SOURCES point sources convolved with it, plus noise."""
    rng = np.random.default_rng(seed)
    d = np.hypot(*np.meshgrid(np.arange(Gp) - Gp // 2, np.arange(Gp) - Gp // 2))
    psf = (0.1 * np.cos(0.7 * d) / (1.0 + 0.05 * d)).astype(np.float32)
    psf[Gp // 2, Gp // 2] = 1.0
    res = (0.01 * rng.normal(size=(G, G))).astype(np.float32)
    for y, x in rng.integers(0, G, (SOURCES, 2)):
        oy, ox = y - Gp // 2, x - Gp // 2
        y0, y1, x0, x1 = max(oy, 0), min(oy + Gp, G), max(ox, 0), min(
            ox + Gp, G)
        res[y0:y1, x0:x1] += np.float32(rng.uniform(1, 10)) * psf[
            y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    return res, psf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clark",
                                                  "rate.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--sizes", default=",".join("%dx%d" % s for s in SIZES))
    args = ap.parse_args()
    import torch
    import idg_amd
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda")
    R, K = args.rounds, args.iterations
    M = R * K
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]

    def timed(fn, restore):
        restore()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3             # us per call

    rows = []
    checked = None
    for G, Gp in sizes:
        res0, psf0 = inputs(G, Gp)
        start = torch.from_numpy(res0).to(dev)
        psf = torch.from_numpy(psf0).to(dev)
        res = start.clone()
        model = torch.zeros_like(res)
        comps = torch.zeros((M, 3), dtype=torch.int32, device=dev)
        kstate = torch.zeros(9, dtype=torch.int32, device=dev)
        cstate = torch.zeros(6, dtype=torch.int32, device=dev)

        def restore():
            res.copy_(start)
            model.zero_()
            kstate.zero_()
            cstate.zero_()

        def clark(rounds=R, per_round=K):
            idg_amd.clark(res, psf, model, gain=GAIN, max_components=M,
                          nr_rounds=rounds, iterations_per_round=per_round,
                          components=comps, state=kstate)

        # round by round, not timed: candidates and components per round
        restore()
        per_round = []
        for _ in range(R):
            before = int(kstate.cpu()[0])
            clark(rounds=1)
            st = kstate.cpu().numpy().view(idg_amd.CLARK_STATE_DTYPE)[0]
            per_round.append({"candidates": int(st["n_candidates"]),
                              "components": int(st["n_components"]) - before,
                              "round_limit": float(st["round_limit"])})
        n = int(st["n_components"])
        reason = int(st["reason"])
        assert n > 0
        if checked is None:
            torch.cuda.synchronize()
            host = idg_amd.clark(
                res0.copy(), psf0, gain=GAIN, max_components=M, nr_rounds=R,
                iterations_per_round=K)
            taken = comps.cpu().numpy().view(
                idg_amd.COMPONENT_DTYPE).reshape(-1)
            checked = {
                "grid_size": G, "psf_size": Gp,
                "residual": res.cpu().numpy().tobytes() == host[0].tobytes(),
                "components": taken.tobytes() == host[2].tobytes()}
            assert checked["residual"] and checked["components"], checked

        def clean():
            idg_amd.clean(res, psf, model, gain=GAIN, max_components=n,
                          nr_iterations=n, components=comps, state=cstate)

        forms = [("clark", clark), ("select", lambda: clark(per_round=0)),
                 ("clean", clean)]
        for _, fn in forms:
            timed(fn, restore)
        us = {name: [] for name, _ in forms}
        for _ in range(args.reps):
            for name, fn in forms:
                us[name].append(timed(fn, restore) / n)
        assert int(kstate.cpu()[0]) == 0 and int(cstate.cpu()[0]) == n
        row = {"grid_size": G, "psf_size": Gp, "components": n,
               "reason": reason, "rounds": per_round,
               "clark_us_per_component": stats(us["clark"]),
               "select_us_per_component": stats(us["select"]),
               "cycle_plus_apply_us_per_component": stats(
                   [a - b for a, b in zip(us["clark"], us["select"])]),
               "clean_us_per_component": stats(us["clean"]),
               "ranges_apart": max(us["clark"]) < min(us["clean"])}
        print(json.dumps(row), flush=True)
        rows.append(row)

    out = {
        "device": idg_amd.device_name(), "reps": args.reps, "rounds": R,
        "iterations_per_round": K, "gain": GAIN, "sources": SOURCES,
        "select_fraction": 0.3, "max_candidates": 4096,
        "timing": "HIP events around one call, us per component taken by the "
                  "clark form; the forms take turns; every window starts from "
                  "the same residual",
        "select": "the clark call with iterations_per_round = 0: all of its "
                  "launches, no component",
        "clean": "idg_amd.clean in the same process for the same number of "
                 "components, one launch each plus two",
        "bytes_equal_host": checked,
        "sizes": rows,
    }
    if args.out == "-":
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
