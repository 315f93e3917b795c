"""The plan step's time at the default batch's extent: 1,225
baselines x 2,560 timesteps of earth-rotation-like tracks, C = 16, S = 32,
G = 1,024, kernel_size 8, at most 128 timesteps per subgrid.

  device  idg_amd.plan_launch on resident uvw, HIP events on the launch
          stream: after a warm-up (code objects, the workspace, clocks), REPS
          windows of LAUNCHES back-to-back launches each, so a window is long
          against the clock's and the scheduler's noise; ms per launch
          (median, min and every window)
  host    idg_amd.plan at 1 and at 16 threads (count + fill), wall clock,
          REPS rounds

and, for the share the plan takes of a gridding step, the gridder's time at
the same batch from a bench line (python bench.py --gpus 1 ... > line.json;
--bench-line line.json), which this tool copies and does not measure.  The
device plan's bytes are checked against the host plan's before anything is
timed.

    python tools/debug/plan_rate.py [--out profiles/plan/rate.json]
                                    [--bench-line FILE] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-idg-bench_amd"))

B, T, C, S, G, K, TMAX = 1225, 2560, 16, 32, 1024, 8, 128
IMAGE_SIZE = 0.01
C_LIGHT = 299792458.0
LAUNCHES = 1000


def tracks(seed=0):
    """Each baseline an arc of the ellipse earth rotation draws: radius
    0.02-0.45 of the grid at the first channel, axis ratio sin(declination),
    2,560 ten-second steps (1.9 rad of hour angle: the short baselines'
    subgrids end at the timestep cap, the long ones' at the subgrid's edge);
    w follows the same rotation."""
    rng = np.random.default_rng(seed)
    wn = (2 * np.pi * (150e6 + 0.2e6 * np.arange(C)) / C_LIGHT).astype(
        np.float32)
    metres_per_cell = 1.0 / (float(wn[0]) / (2 * np.pi) * IMAGE_SIZE)
    r = rng.uniform(0.02, 0.45, (B, 1)) * G * metres_per_cell
    h0 = rng.uniform(0, 2 * np.pi, (B, 1))
    tilt = rng.uniform(0, np.pi, (B, 1))
    sin_dec = np.sin(np.deg2rad(50.0))
    h = h0 + 2 * np.pi * 10.0 * np.arange(T)[None, :] / 86164.0
    ex, ey = r * np.cos(h), r * sin_dec * np.sin(h)
    uvw = np.empty((B, T, 3), np.float32)
    uvw[..., 0] = ex * np.cos(tilt) - ey * np.sin(tilt)
    uvw[..., 1] = ex * np.sin(tilt) + ey * np.cos(tilt)
    uvw[..., 2] = 0.05 * r * np.cos(h + 1.0)
    st = np.array([(i, j) for i in range(50) for j in range(i + 1, 50)],
                  np.int32)
    assert st.shape[0] == B
    return uvw, st, wn


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)),
            "all": [round(float(x), 5) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "plan",
                                                  "rate.json"))
    ap.add_argument("--bench-line", default=None)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import idg_amd
    assert torch.cuda.is_available(), "needs a HIP device"
    uvw, bl, wn = tracks()
    p = (G, S, IMAGE_SIZE, 0.0, uvw, bl, wn, K, TMAX)

    host = {}
    for nthreads in (1, 16):
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            md, dropped = idg_amd.plan(*p, nthreads=nthreads)
            ms.append((time.perf_counter() - t0) * 1e3)
        host[f"{nthreads}_threads_ms"] = stats(ms)

    d_uvw, d_bl, d_wn = (torch.from_numpy(a).cuda() for a in (uvw, bl, wn))
    d_md = torch.zeros((B * T // 8, 9), dtype=torch.int32, device="cuda")
    assert md.size <= d_md.shape[0]

    def launch():
        return idg_amd.plan_launch(G, S, IMAGE_SIZE, 0.0, d_uvw, d_bl, d_wn,
                                   K, TMAX, metadata=d_md)

    _, counts = launch()
    assert tuple(counts.cpu().numpy()) == (md.size, dropped)
    assert np.array_equal(d_md[:md.size].cpu().numpy(),
                          md.view(np.int32).reshape(-1, 9))
    for _ in range(LAUNCHES):           # warm-up
        launch()
    torch.cuda.synchronize()
    dev = []
    for _ in range(args.reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            launch()
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) / LAUNCHES)

    res = {
        "device": idg_amd.device_name(), "reps": args.reps,
        "shape": dict(nr_baselines=B, nr_timesteps=T, nr_channels=C,
                      subgrid_size=S, grid_size=G, kernel_size=K,
                      max_nr_timesteps_per_subgrid=TMAX,
                      uvw_bytes=int(uvw.nbytes)),
        "subgrids": int(md.size), "dropped_timesteps": int(dropped),
        "timesteps_per_subgrid": {"mean": float(md["nr_timesteps"].mean()),
                                  "min": int(md["nr_timesteps"].min()),
                                  "max": int(md["nr_timesteps"].max())},
        "device_plan_ms": dict(stats(dev), launches_per_window=LAUNCHES,
                               timing="HIP events around back-to-back "
                                      "plan_launch calls, per launch"),
        "host_plan_ms": dict(host, timing="wall clock around idg_amd.plan "
                                          "(count + fill), uvw in host "
                                          "memory; no copies included"),
    }
    if args.bench_line:
        with open(args.bench_line) as f:
            line = [ln for ln in f if ln.lstrip().startswith("{")][-1]
        g_ms = json.loads(line)["kernels"]["gridder"]["ms"]
        res["gridder_ms_same_batch"] = {
            "ms": g_ms, "source": "kernels.gridder.ms of the bench line "
            "(24,500 subgrids of 128 timesteps: the same 1,225 x 2,560 rows)"}
        res["plan_share_of_gridder"] = {
            "device": res["device_plan_ms"]["median"] / g_ms,
            "host_1_thread": host["1_threads_ms"]["median"] / g_ms,
            "host_16_threads": host["16_threads_ms"]["median"] / g_ms}
    print(json.dumps({k: res[k] for k in res if k != "shape"}))
    if args.out == "-":
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
