"""Multi-scale CLEAN's times, measured, not gated.

Iteration: G = 1024, 2048, 4096, each with Gp = 256 and Gp = G, at Ns = 1
(scales (0,)), 4 ((0, 4, 8, 16)) and 6 ((0, 4, 8, 16, 32, 64)); us per
iteration of idg_amd.ms_clean on prepared planes, beside

  clean     idg_amd.clean's iteration at the same G and Gp in the same process
            (on the same residual and PSF): the yardstick
  floor     12 bytes (plane read and written, cross-PSF read) per pixel of the
            patch intersected with the image, times Ns, averaged over the
            components the run took, over the 8 TB/s the bench line uses

Prepare: the convolution in ms per plane at the same G for r = 3, 12 and 48
(scales 4, 21 and 85), beside the floor of 8 bytes per pixel per pass (two
passes); and ms_prepare as a whole for the six scales at Gp = 256.

HIP events around windows of one call of ITERATIONS iterations (CALLS
convolutions); REPS windows of each form taking turns after a warm-up window;
median, min and max.  Every iteration window starts from the same planes
(restored before the first event, not timed).  The device's bytes are checked
against the host entries' at G = 1024, Gp = 256, Ns = 4 before anything is
timed.

    python tools/debug/multiscale_rate.py [--out profiles/multiscale/rate.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clean_rate import HBM_PEAK_GBS, patch_bytes, stats  # noqa: E402

SIZES = [(1024, 256), (1024, 1024), (2048, 256), (2048, 2048), (4096, 256),
         (4096, 4096)]
SCALES = {1: (0,), 4: (0, 4, 8, 16), 6: (0, 4, 8, 16, 32, 64)}
CONV_SCALES = (4, 21, 85)      # r = 3, 12, 48
GAIN = 0.1
CALLS = 10


def inputs(G, Gp, seed=1):
    """A PSF with a sigma = 1.2 main lobe and damped cosine sidelobes (centre
    1), and a residual of 64 point sources convolved with it, plus noise."""
    rng = np.random.default_rng(seed)
    d = np.hypot(*np.meshgrid(np.arange(Gp) - Gp // 2, np.arange(Gp) - Gp // 2))
    lobe = np.exp(-d ** 2 / (2 * 1.2 ** 2))
    psf = (lobe + 0.05 * np.cos(0.9 * d) * np.exp(-d / 10.0)
           * (1 - lobe)).astype(np.float32)
    res = (0.01 * rng.normal(size=(G, G))).astype(np.float32)
    for y, x in rng.integers(0, G, (64, 2)):
        oy, ox = y - Gp // 2, x - Gp // 2
        y0, y1, x0, x1 = max(oy, 0), min(oy + Gp, G), max(ox, 0), min(
            ox + Gp, G)
        res[y0:y1, x0:x1] += np.float32(rng.uniform(1, 10)) * psf[
            y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    return res, psf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "multiscale", "rate.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=200)
    args = ap.parse_args()
    import torch
    import idg_amd
    assert torch.cuda.is_available(), "needs a HIP device"
    assert args.iterations >= 200, "at least 200 iterations per window"
    N = args.iterations
    dev = torch.device("cuda")

    def timed(fn, restore, per):
        restore()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / per      # us per unit

    def take_turns(forms, restore, per):
        for _, fn in forms:
            timed(fn, restore, per)
        us = {name: [] for name, _ in forms}
        for _ in range(args.reps):
            for name, fn in forms:
                us[name].append(timed(fn, restore, per))
        return us

    iteration_rows, convolution_rows, prepare_rows = [], [], []
    checked = None
    for G, Gp in SIZES:
        res0, psf0 = inputs(G, Gp)
        start = torch.from_numpy(res0).to(dev)
        psf = torch.from_numpy(psf0).to(dev)
        res = start.clone()
        model = torch.zeros_like(res)
        comps = torch.zeros((N, 3), dtype=torch.int32, device=dev)
        state = torch.zeros(6, dtype=torch.int32, device=dev)
        tmp = torch.empty_like(res)
        runs = {}
        for Ns, scales in SCALES.items():
            taps = idg_amd.ms_scale_taps(scales)
            planes0, cross = idg_amd.ms_prepare(start, psf, taps, tmp=tmp)
            weight, inv_peak = idg_amd.ms_weights(cross, scales)
            runs[Ns] = dict(
                taps=taps, planes0=planes0, cross=cross, weight=weight,
                inv_peak=inv_peak, planes=planes0.clone(),
                comps=torch.zeros((N, 4), dtype=torch.int32, device=dev),
                state=torch.zeros(7, dtype=torch.int32, device=dev))

        def restore():
            res.copy_(start)
            model.zero_()
            state.zero_()
            for r in runs.values():
                r["planes"].copy_(r["planes0"])
                r["state"].zero_()

        def hogbom():
            idg_amd.clean(res, psf, model, gain=GAIN, max_components=N,
                          nr_iterations=N, components=comps, state=state)

        def multiscale(Ns):
            r = runs[Ns]

            def run():
                idg_amd.ms_clean(r["planes"], r["cross"], r["taps"],
                                 r["weight"], r["inv_peak"], model=model,
                                 gain=GAIN, max_components=N, nr_iterations=N,
                                 components=r["comps"], state=r["state"])
            return run

        # the components each form takes, for the floors; at the first size
        # the bytes against the host entries'
        floors = {}
        for Ns in SCALES:
            restore()
            multiscale(Ns)()
            torch.cuda.synchronize()
            r = runs[Ns]
            taken = r["comps"].cpu().numpy().view(
                idg_amd.MS_COMPONENT_DTYPE).reshape(-1)
            st = r["state"].cpu().numpy().view(idg_amd.MS_STATE_DTYPE)[0]
            assert st["n_components"] == N and st["reason"] == 0, st
            floors[Ns] = (Ns * patch_bytes(
                [(c["y"], c["x"], 0) for c in taken], G, Gp) / N
                / (HBM_PEAK_GBS * 1e9) * 1e6)
            if checked is None and Ns == 4:
                hp, hc = idg_amd.ms_prepare(res0, psf0, r["taps"])
                prepared = (r["planes0"].cpu().numpy().tobytes()
                            == hp.tobytes()
                            and r["cross"].cpu().numpy().tobytes()
                            == hc.tobytes())
                host = idg_amd.ms_clean(hp, hc, r["taps"], r["weight"],
                                        r["inv_peak"], gain=GAIN,
                                        max_components=N, nr_iterations=N)
                checked = {
                    "grid_size": G, "psf_size": Gp, "scales": SCALES[4],
                    "prepare": prepared,
                    "planes": r["planes"].cpu().numpy().tobytes()
                    == host[0].tobytes(),
                    "model": model.cpu().numpy().tobytes()
                    == host[1].tobytes(),
                    "components": taken.tobytes() == host[2].tobytes()}
                assert all(v for k, v in checked.items()
                           if isinstance(v, bool)), checked
        forms = [("clean", hogbom)] + [("ns%d" % Ns, multiscale(Ns))
                                       for Ns in SCALES]
        us = take_turns(forms, restore, N)
        row = {"grid_size": G, "psf_size": Gp,
               "clean_us": stats(us["clean"])}
        for Ns in SCALES:
            row["ns%d_us" % Ns] = stats(us["ns%d" % Ns])
            row["ns%d_floor_us" % Ns] = round(floors[Ns], 3)
            row["ns%d_over_clean" % Ns] = round(
                float(np.median(us["ns%d" % Ns]) / np.median(us["clean"])), 3)
        print(json.dumps(row), flush=True)
        iteration_rows.append(row)

        if Gp == 256:
            out = torch.empty_like(res)
            conv_taps = [torch.from_numpy(t).to(dev)
                         for t in idg_amd.ms_scale_taps(CONV_SCALES)]

            def conv(t):
                def run():
                    for _ in range(CALLS):
                        idg_amd.convolve_separable(start, t, out=out, tmp=tmp)
                return run

            def whole():
                r = runs[6]
                idg_amd.ms_prepare(start, psf, r["taps"], planes=r["planes"],
                                   cross_psf=r["cross"], tmp=tmp)
            us = take_turns([("r%d" % (t.numel() // 2), conv(t))
                             for t in conv_taps], lambda: None, CALLS)
            crow = {"grid_size": G,
                    "floor_ms": round(16.0 * G * G / (HBM_PEAK_GBS * 1e9)
                                      * 1e3, 4)}
            for name, v in us.items():
                crow[name + "_ms"] = stats([u * 1e-3 for u in v])
            print(json.dumps(crow), flush=True)
            convolution_rows.append(crow)
            us = take_turns([("prepare", whole)], lambda: None, 1)
            prow = {"grid_size": G, "psf_size": Gp, "scales": SCALES[6],
                    "ms": stats([u * 1e-3 for u in us["prepare"]])}
            print(json.dumps(prow), flush=True)
            prepare_rows.append(prow)
        del runs

    out = {
        "device": idg_amd.device_name(), "reps": args.reps,
        "iterations_per_window": N, "gain": GAIN,
        "timing": "HIP events around one call of iterations_per_window "
                  "iterations (search + iterations + finish launches), us per "
                  "iteration; the forms take turns; every window starts from "
                  "the same planes.  Convolutions: windows of %d calls, ms "
                  "per call; ms_prepare: one call per window" % CALLS,
        "hbm_peak_gbs": HBM_PEAK_GBS,
        "floor": "iteration: 12 bytes per pixel of the patch inside the "
                 "image times Ns, averaged over the components taken; "
                 "convolution: 8 bytes per pixel per pass, two passes",
        "scales": {str(k): v for k, v in SCALES.items()},
        "convolution_radii": "r = 3, 12, 48 (scales 4, 21, 85)",
        "bytes_equal_host": checked,
        "iteration": iteration_rows,
        "convolution": convolution_rows,
        "prepare": prepare_rows,
    }
    if args.out == "-":
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
