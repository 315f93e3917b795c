"""The Hogbom minor cycle's time per iteration, measured, not
gated: G = 1024, 2048, 4096, each with a PSF as large as the image and with
Gp = 256.

  carry     idg_amd.clean as shipped: a tile the patch does not touch carries
            its partial forward
  rescan    the same with IDG_CLEAN_RESCAN=1: every tile rescans
  torch     the same iteration restated in torch in the same process:
            abs().argmax(), then an in-place slice sub_ of gain * peak * psf.
            torch needs the peak's position on the host to form the slices, so
            there is one .item() per iteration (on the argmax); the peak value
            stays on the device.  No mask, no stop test, no component record.
  idle      one launch of a stopped run (reason != 0): a call of ITERATIONS
            iterations on a state whose reason is already set, less a call of
            none, per iteration

each iteration beside its floor: 12 bytes (residual read and written, PSF
read) per pixel of the patch intersected with the image, summed over the
components the run took, over the 8 TB/s the bench line uses.

HIP events around windows of one call of ITERATIONS iterations; REPS windows
of each form taking turns after a warm-up window; median, min and max per
iteration.  Every window starts from the same residual (restored before the
first event, not timed).  The device's bytes are checked against the host
entry's at G = 1024 before anything is timed.

    python tools/debug/clean_rate.py [--out profiles/clean/rate.json]
                                     [--reps 7] [--iterations 200]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-idg-bench_amd"))

HBM_PEAK_GBS = 8000.0     # as bench.py
SIZES = [(1024, 1024), (1024, 256), (2048, 2048), (2048, 256), (4096, 4096),
         (4096, 256)]
GAIN = 0.1


def stats(us):
    return {"median": round(float(np.median(us)), 3),
            "min": round(float(min(us)), 3), "max": round(float(max(us)), 3)}


def inputs(G, Gp, seed=1):
    """A smooth PSF (centre 1, sidelobes falling off from 0.3) and a residual
    of 64 point sources convolved with it, plus noise."""
    rng = np.random.default_rng(seed)
    d = np.hypot(*np.meshgrid(np.arange(Gp) - Gp // 2, np.arange(Gp) - Gp // 2))
    psf = (0.3 * np.cos(0.7 * d) / (1.0 + 0.05 * d)).astype(np.float32)
    psf[Gp // 2, Gp // 2] = 1.0
    res = (0.01 * rng.normal(size=(G, G))).astype(np.float32)
    for y, x in rng.integers(0, G, (64, 2)):
        oy, ox = y - Gp // 2, x - Gp // 2
        y0, y1, x0, x1 = max(oy, 0), min(oy + Gp, G), max(ox, 0), min(
            ox + Gp, G)
        res[y0:y1, x0:x1] += np.float32(rng.uniform(1, 10)) * psf[
            y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    return res, psf


def tile_rows(G):
    """Rows of a tile (kernels/minor_cycle.hpp tiling_of): 256 columns wide, at
    least 8 rows, at most 2048 tiles."""
    tiles_x = -(-G // 256)
    return max(8, -(-G // (2048 // tiles_x)))


def patch_bytes(components, G, Gp):
    """12 bytes per pixel of each component's patch inside the image."""
    total = 0
    for y, x, _ in components:
        oy, ox = int(y) - Gp // 2, int(x) - Gp // 2
        total += 12 * (min(oy + Gp, G) - max(oy, 0)) * (
            min(ox + Gp, G) - max(ox, 0))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clean",
                                                  "rate.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=200)
    args = ap.parse_args()
    import torch
    import idg_amd
    assert torch.cuda.is_available(), "needs a HIP device"
    assert args.iterations >= 200, "at least 200 iterations per window"
    N = args.iterations
    dev = torch.device("cuda")

    def timed(fn, restore):
        restore()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / N      # us per iteration

    rows = []
    checked = None
    for G, Gp in SIZES:
        res0, psf0 = inputs(G, Gp)
        start = torch.from_numpy(res0).to(dev)
        psf = torch.from_numpy(psf0).to(dev)
        res = start.clone()
        model = torch.zeros_like(res)
        comps = torch.zeros((N, 3), dtype=torch.int32, device=dev)
        state = torch.zeros(6, dtype=torch.int32, device=dev)

        def restore():
            res.copy_(start)
            model.zero_()
            state.zero_()

        def device(rescan):
            def run():
                os.environ["IDG_CLEAN_RESCAN"] = rescan
                idg_amd.clean(res, psf, model, gain=GAIN, max_components=N,
                              nr_iterations=N, components=comps, state=state)
            return run

        def idle():
            # a stopped run: every launch returns after reading the state
            state[1] = 3
            idg_amd.clean(res, psf, model, gain=GAIN, max_components=N,
                          nr_iterations=N, components=comps, state=state)

        def none():
            state[1] = 3
            idg_amd.clean(res, psf, model, gain=GAIN, max_components=N,
                          nr_iterations=0, components=comps, state=state)

        def torch_form():
            half = Gp // 2
            for _ in range(N):
                i = int(res.abs().argmax().item())     # the one forced sync
                py, px = divmod(i, G)
                oy, ox = py - half, px - half
                y0, y1 = max(oy, 0), min(oy + Gp, G)
                x0, x1 = max(ox, 0), min(ox + Gp, G)
                c = res[py, px] * GAIN                 # stays on the device
                res[y0:y1, x0:x1].sub_(
                    c * psf[y0 - oy:y1 - oy, x0 - ox:x1 - ox])

        # the components of the shipped form, for the floor; at the first
        # size the bytes against the host entry's
        restore()
        device("0")()
        torch.cuda.synchronize()
        taken = comps.cpu().numpy().view(idg_amd.COMPONENT_DTYPE).reshape(-1)
        n = int(state.cpu()[0])
        assert n == N and int(state.cpu()[1]) == 0
        if checked is None:
            host = idg_amd.clean(res0.copy(), psf0, gain=GAIN,
                                 max_components=N, nr_iterations=N)
            checked = {
                "grid_size": G, "psf_size": Gp,
                "residual": res.cpu().numpy().tobytes() == host[0].tobytes(),
                "components": taken.tobytes() == host[2].tobytes()}
            assert checked["residual"] and checked["components"], checked
        floor_us = patch_bytes(taken[:n], G, Gp) / n / (HBM_PEAK_GBS * 1e9) * 1e6

        forms = [("carry", device("0")), ("rescan", device("1")),
                 ("torch", torch_form), ("idle", idle), ("none", none)]
        for _, fn in forms:
            timed(fn, restore)
        us = {name: [] for name, _ in forms}
        for _ in range(args.reps):
            for name, fn in forms:
                us[name].append(timed(fn, restore))
        os.environ.pop("IDG_CLEAN_RESCAN", None)
        idle_us = [a - b for a, b in zip(us["idle"], us["none"])]
        row = {"grid_size": G, "psf_size": Gp,
               "tiles": "256 columns x %d rows" % tile_rows(G),
               "hbm_floor_us": round(floor_us, 3),
               "carry_us": stats(us["carry"]), "rescan_us": stats(us["rescan"]),
               "torch_us": stats(us["torch"]),
               "idle_launch_us": stats(idle_us)}
        print(json.dumps(row), flush=True)
        rows.append(row)

    out = {
        "device": idg_amd.device_name(), "reps": args.reps,
        "iterations_per_window": N, "gain": GAIN,
        "timing": "HIP events around one call of iterations_per_window "
                  "iterations (search + iterations + finish launches), us per "
                  "iteration; the forms take turns; every window starts from "
                  "the same residual",
        "hbm_peak_gbs": HBM_PEAK_GBS,
        "floor": "12 bytes per pixel of the patch inside the image, averaged "
                 "over the components taken",
        "torch": "abs().argmax() then an in-place slice sub_; one .item() per "
                 "iteration, on the argmax (the slice bounds are host "
                 "integers); no mask, no stop test, no component record",
        "idle_launch": "a call of iterations_per_window launches on a stopped "
                       "state less a call of none, per launch",
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
