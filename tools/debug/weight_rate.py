"""The imaging-weight steps' time, measured, not gated, at the
perf defaults' extent: plan_rate.py's 1,225 x 2,560 rows of planned tracks
(about 24,500 subgrids of up to 128 timesteps), C = 16, S = 32, G = 1,024.

  density   idg_amd.weight_density with the S x S LDS tile, and the same
            kernel with every sample sent down the global-atomic path
            (IDG_WEIGHT_TILE=0), their windows alternating
  scheme    idg_amd.weight_scheme, Briggs (the two-stage sum over G^2 cells)
  apply     idg_amd.weight_apply, out of place

each beside the bytes it must move over the peak the bench line uses
(8 TB/s), the density also beside torch.Tensor.index_put_(accumulate=True) on
a float64 grid with the cell indices and the weights precomputed (not timed),
and the three steps' sum as a share of the gridder's time from
idg_amd.p_run_gridder() in the same process (the perf defaults: 24,500
subgrids of 128 timesteps, the same number of samples).

HIP events around windows of LAUNCHES back-to-back calls after a warm-up;
REPS windows of each; median, min and max per call.  The device density is
checked against the host's before anything is timed.

    python tools/debug/weight_rate.py [--out profiles/weight/rate.json]
                                      [--reps 7]
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

import plan_rate as pr  # noqa: E402

HBM_PEAK_GBS = 8000.0     # as bench.py
LAUNCHES = 10


def stats(ms):
    return {"median": round(float(np.median(ms)), 5),
            "min": round(float(min(ms)), 5), "max": round(float(max(ms)), 5)}


def window(fn):
    import torch
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


def alternating(fns, reps):
    """REPS windows of each of `fns`, taking turns, after a warm-up window."""
    for fn in fns:
        window(fn)
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(window(fn))
    return [stats(m) for m in ms]


def floor_ms(nbytes):
    return round(nbytes / (HBM_PEAK_GBS * 1e9) * 1e3, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "weight",
                                                  "rate.json"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import idg_amd
    assert torch.cuda.is_available(), "needs a HIP device"
    G, S, C = pr.G, pr.S, pr.C
    uvw, bl, wn = pr.tracks()
    md, dropped = idg_amd.plan(G, S, pr.IMAGE_SIZE, 0.0, uvw, bl, wn, pr.K,
                               pr.TMAX, nthreads=16)
    rows = pr.B * pr.T
    rng = np.random.default_rng(1)
    weights = rng.uniform(0.25, 4.0, (rows, C)).astype(np.float32)
    host = idg_amd.weight_density(G, S, pr.IMAGE_SIZE, uvw.reshape(-1, 3), wn,
                                  weights, md)

    dev = torch.device("cuda")
    t_uvw = torch.from_numpy(uvw.reshape(-1, 3)).to(dev)
    t_wn = torch.from_numpy(wn).to(dev)
    t_w = torch.from_numpy(weights).to(dev)
    t_md = torch.from_numpy(md.view(np.int32).reshape(-1, 9)).to(dev)
    vis = torch.randn((rows, C, 4, 2), device=dev)
    out = torch.empty_like(vis)
    iw = torch.empty((rows, C), device=dev)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    ab = torch.zeros(2, device=dev)
    density = torch.zeros((G, G), dtype=torch.int64, device=dev)

    def dens(tile):
        def run():
            os.environ["IDG_WEIGHT_TILE"] = tile
            idg_amd.weight_density(G, S, pr.IMAGE_SIZE, t_uvw, t_wn, t_w,
                                   t_md, density)
        return run

    same = {}
    for tile in ("1", "0"):
        density.zero_()
        dens(tile)()
        same[tile] = bool(np.array_equal(
            density.cpu().numpy().view(np.uint64), host))
    assert all(same.values()), same

    # torch's scatter-add of the same samples onto a float64 grid
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import weight_cases as wc
    q, X, Y = wc.sample_q(G, pr.IMAGE_SIZE, uvw.reshape(-1, 3), wn, weights)
    live = (q > 0) & (wc.cover(md, rows) > 0)[:, None]
    idx = torch.from_numpy((Y * G + X)[live]).to(dev)
    val = torch.from_numpy(weights[live].astype(np.float64)).to(dev)
    fgrid = torch.zeros(G * G, dtype=torch.float64, device=dev)

    def torch_density():
        fgrid.index_put_((idx,), val, accumulate=True)

    d_tile, d_global, d_torch = alternating(
        [dens("1"), dens("0"), torch_density], args.reps)
    os.environ.pop("IDG_WEIGHT_TILE", None)

    density.zero_()
    idg_amd.weight_density(G, S, pr.IMAGE_SIZE, t_uvw, t_wn, t_w, t_md,
                           density)
    (scheme,) = alternating(
        [lambda: idg_amd.weight_scheme(G, density, "briggs", 0.0, ab=ab)],
        args.reps)
    (apply_,) = alternating(
        [lambda: idg_amd.weight_apply(G, pr.IMAGE_SIZE, t_uvw, t_wn, t_w,
                                      t_md, density, ab, vis, iw, out,
                                      total)], args.reps)
    covered = int(md["nr_timesteps"].sum())
    gridder_ms = float(idg_amd.p_run_gridder())
    steps = d_tile["median"] + scheme["median"] + apply_["median"]
    res = {
        "device": idg_amd.device_name(), "reps": args.reps,
        "launches_per_window": LAUNCHES,
        "timing": "HIP events around windows of back-to-back calls, ms per "
                  "call; the density's three forms take turns",
        "hbm_peak_gbs": HBM_PEAK_GBS,
        "shape": dict(nr_baselines=pr.B, nr_timesteps=pr.T, nr_channels=C,
                      subgrid_size=S, grid_size=G, subgrids=int(md.size),
                      covered_rows=covered, dropped_timesteps=int(dropped),
                      samples=covered * C),
        "density_bytes_equal_host": same,
        "density_ms": {
            "lds_tile": d_tile, "all_global_atomics": d_global,
            "torch_index_put_float64": d_torch,
            "hbm_floor_ms": floor_ms(covered * (12 + 4 * C)),
            "floor": "uvw rows + weights read once; the atomics' bytes not "
                     "counted"},
        "scheme_briggs_ms": {"ms": scheme,
                             "hbm_floor_ms": floor_ms(G * G * 8),
                             "floor": "the density read once"},
        "apply_ms": {"ms": apply_,
                     "hbm_floor_ms": floor_ms(covered * (12 + C * (4 + 4 + 64))
                                              + G * G * 8),
                     "floor": "uvw, weights, visibilities read; imaging "
                              "weights, weighted visibilities written; the "
                              "density once"},
        "p_run_gridder_ms": gridder_ms,
        "three_steps_ms": round(steps, 5),
        "three_steps_share_of_gridder": round(steps / gridder_ms, 4),
    }
    print(json.dumps(res))
    if args.out == "-":
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
