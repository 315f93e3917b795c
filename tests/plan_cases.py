"""Inputs of the plan step's tests (test_plan_host.py on the CPU,
test_gpu_plan.py on the GPU): uvw tracks that are arcs of ellipses, and the
on-cell case that pins the conventions end to end."""
import numpy as np

import pipeline_oracle as pl

F = np.float32
C_LIGHT = 299792458.0
IMAGE_SIZE = 0.01

# (w_step_in_lambda, nr_w_layers, nr_timesteps_per_aterm, max per subgrid)
VARIANTS = [(0.0, 1, 0, 128), (8.0, 4, 0, 128), (0.0, 1, 64, 128),
            (8.0, 4, 50, 128), (0.0, 1, 0, 1)]


def wavenumbers(C, f0=150e6, df=0.7e6):
    return (2.0 * np.pi * (f0 + df * np.arange(C)) / C_LIGHT).astype(F)


def arc_tracks(B, T, G, C=8, seed=1, bad_rows=True):
    """Arcs of ellipses around the grid centre, radii 0.05-0.40 of G (in uv
    cells at the first channel), a per-baseline w of 0-40 m plus a 0-20 m
    ramp; with bad_rows one NaN row and three consecutive rows at u = 1e7.
    Returns uvw [B, T, 3] f32 (metres), baselines [B, 2] i32, wn [C] f32."""
    rng = np.random.default_rng(seed)
    wn = wavenumbers(C)
    metres_per_cell = 1.0 / (float(wn[0]) / (2 * np.pi) * IMAGE_SIZE)
    uvw = np.zeros((B, T, 3), np.float64)
    for bl in range(B):
        ra, rb = rng.uniform(0.05, 0.40, 2) * G
        a0 = rng.uniform(0, 2 * np.pi)
        span = rng.uniform(0.3, 1.6) * (1 if bl % 2 else -1)
        tilt = rng.uniform(0, np.pi)
        if bl == 0:     # a slow one: its subgrids end at the timestep cap
            ra, rb, span = 0.05 * G, 0.06 * G, 0.25
        ang = a0 + span * np.arange(T) / max(T - 1, 1)
        ex, ey = ra * np.cos(ang), rb * np.sin(ang)
        uvw[bl, :, 0] = (ex * np.cos(tilt) - ey * np.sin(tilt)) * metres_per_cell
        uvw[bl, :, 1] = (ex * np.sin(tilt) + ey * np.cos(tilt)) * metres_per_cell
        uvw[bl, :, 2] = rng.uniform(0, 40) + rng.uniform(0, 20) * \
            np.arange(T) / max(T - 1, 1)
    uvw = uvw.astype(F)
    if bad_rows:
        uvw[min(3, B - 1), T // 3, 1] = np.nan
        uvw[min(7, B - 1), T // 2:T // 2 + 3, 0] = 1e7
    st = np.array([(i, j) for i in range(64) for j in range(i + 1, 64)],
                  np.int32)
    return uvw, np.ascontiguousarray(st[:B]), wn


# ---- the on-cell case: conventions end to end -----------------------------
ONCELL = dict(G=256, S=32, K=8, Tmax=48, B=6, T=96, image_size=1.0 / 64)


def oncell_case():
    """C = 1, wavenumber 2 pi, image_size 1/64: u = (Ux - G/2) * 64 puts
    every visibility exactly on uv cell (Ux, Uy).  Slow tracks (several
    visibilities per cell), unit xx / yy visibilities, identity A-terms,
    taper 1.  Returns a dict of arrays and the [G, G] histogram of cells."""
    G, S, B, T = (ONCELL[k] for k in ("G", "S", "B", "T"))
    rng = np.random.default_rng(5)
    cells = np.zeros((B, T, 2), np.int64)
    for bl in range(B):
        r = rng.uniform(0.08, 0.38) * G
        a0 = rng.uniform(0, 2 * np.pi)
        ang = a0 + rng.uniform(0.05, 0.6) * np.arange(T) / T
        cells[bl, :, 0] = np.rint(G / 2 + r * np.cos(ang))
        cells[bl, :, 1] = np.rint(G / 2 + 0.7 * r * np.sin(ang))
    uvw = np.zeros((B, T, 3), F)
    uvw[..., :2] = (cells - G // 2) * 64.0
    st = 4
    base = np.array([(i, j) for i in range(st) for j in range(i + 1, st)],
                    np.int32)[:B]
    vis = np.zeros((B * T, 1, 4, 2), F)
    vis[:, :, 0, 0] = 1.0
    vis[:, :, 3, 0] = 1.0
    at = np.zeros((1, st, S, S, 4, 2), F)
    at[..., 0, 0] = 1.0
    at[..., 3, 0] = 1.0
    hist = np.zeros((G, G), np.int64)
    np.add.at(hist, (cells[..., 1].ravel(), cells[..., 0].ravel()), 1)
    return dict(uvw=uvw, baselines=np.ascontiguousarray(base),
                wn=np.array([2 * np.pi], F), vis=vis, aterms=at,
                spheroidal=np.ones((S, S), F), nr_stations=st, hist=hist)


def oncell_grid_through_the_oracle(oracle_lib, case, md):
    """plan's metadata -> oracle gridder -> subgrid FFT (+1) -> adder."""
    o = ONCELL
    sg = np.zeros((md.size, 4, o["S"], o["S"], 2), F)
    oracle_lib.gridder(md.size, o["G"], o["S"], o["image_size"], 0.0, 1,
                       case["nr_stations"], case["uvw"], case["wn"],
                       case["vis"], case["spheroidal"], case["aterms"], md, sg)
    return pl.adder(np.zeros((1, 4, o["G"], o["G"]), complex), md,
                    pl.subgrid_fft(pl.to_complex(sg), +1))
