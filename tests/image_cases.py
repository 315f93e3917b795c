"""Inputs and checkers of the grid <-> image tests (test_image_host.py on the
CPU, test_gpu_image.py on the GPU): a numpy restatement of the
grid_to_image / image_to_grid arithmetic with the constants §13 derives, the
oracle chains it completes (visibilities -> image, image -> visibilities) and
the direct sums of the contract they are checked against."""
import numpy as np

import pipeline_oracle as pl
import plan_cases as pc

F = np.float32


# ---- the restatement -------------------------------------------------------
def lm(G, image_size, dtype=np.float64):
    """l (or m) of the image pixels: (x - G/2) image_size / G."""
    return ((np.arange(G) - G // 2).astype(dtype)
            * dtype(image_size) / dtype(G))


def n_of(l, m):
    """1 - sqrt(1 - l^2 - m^2) in the cancellation-free form of the
    kernels, broadcast over m[:, None], l[None, :]."""
    tmp = m[:, None] * m[:, None] + l[None, :] * l[None, :]
    one = tmp.dtype.type(1)
    return np.where(tmp > 1, one, tmp / (one + np.sqrt(one - np.minimum(tmp, one))))


def w_phasors(G, W, image_size, w_step, sign, single=False):
    """exp(sign 2 pi i w_step (z + 0.5) n(l, m)) as [W, G, G]; single: every
    step in float32 / complex64, as a straightforward f32 kernel would."""
    real = F if single else np.float64
    l = lm(G, image_size, real)
    n = n_of(l, l)
    z = (np.arange(W).astype(real) + real(0.5))[:, None, None]
    phase = real(sign) * real(2 * np.pi) * real(w_step) * z * n[None]
    out = np.cos(phase) + 1j * np.sin(phase)
    return out.astype(np.complex64 if single else np.complex128)


def centre_flip(G):
    """(-1)^(x + y): the fftshift of an even-sized transform, as a factor."""
    s = 1 - 2 * (np.arange(G) % 2)
    return (s[:, None] * s[None, :]).astype(np.float64)


def grid_to_image(grid, image_size, w_step, correction=None, single=False):
    """complex grid [W, 4, G, G] -> image [4, G, G]:
    correction * sum_z conj(w phasor z) * flip * fft2(flip * grid[z])
    (sign -1, unscaled; no phase ramp, no factor of G)."""
    W, _, G, _ = grid.shape
    ctype = np.complex64 if single else np.complex128
    flip = centre_flip(G).astype(F if single else np.float64)
    ph = w_phasors(G, W, image_size, w_step, -1, single)
    f = np.fft.fft2((grid.astype(ctype) * flip).astype(ctype), axes=(-2, -1))
    f = (f.astype(ctype) * flip).astype(ctype)
    image = (f * ph[:, None]).astype(ctype).sum(axis=0, dtype=ctype)
    if correction is not None:
        image = image * correction.astype(F if single else np.float64)
    return image.astype(ctype)


def image_to_grid(image, W, image_size, w_step, correction=None,
                  single=False):
    """The exact adjoint: grid[z] = flip * G^2 ifft2(flip * w phasor z *
    correction * image) (sign +1, unscaled)."""
    G = image.shape[-1]
    ctype = np.complex64 if single else np.complex128
    real = F if single else np.float64
    flip = centre_flip(G).astype(real)
    ph = w_phasors(G, W, image_size, w_step, +1, single)
    src = image.astype(ctype)
    if correction is not None:
        src = (src * correction.astype(real)).astype(ctype)
    src = (src * flip).astype(ctype)
    x = (src[None] * ph[:, None]).astype(ctype)
    g = np.fft.ifft2(x, axes=(-2, -1)).astype(ctype) * real(G * G)
    return (g * flip).astype(ctype)


def rel_max(a, b):
    """max |a - b| over max |b|."""
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- the small end-to-end case ---------------------------------------------
SMALL = dict(G=128, S=32, K=12, C=2, B=4, T=48, image_size=0.1, Tmax=32)


def kaiser_taper(S, beta=9.0):
    """A separable Kaiser-Bessel window sampled at the subgrid's half-pixel
    positions: its transform falls below 1e-3 of the peak about four uv cells
    out, inside the K / 2 cells the plan keeps free.  (The generator's
    `spheroidal` is a test ramp |x| |y| that vanishes at the field centre; it
    tapers nothing, so the error bound asked of these inputs needs another.)"""
    a = (np.arange(S) + 0.5 - S // 2) / (S / 2.0)
    w = np.i0(beta * np.sqrt(1.0 - a * a)) / np.i0(beta)
    return np.ascontiguousarray(np.outer(w, w).astype(F))


def small_case(W, w_step, seed=3):
    """A few baselines on slow arcs well inside the grid, w spread over the
    W layers (w_step in wavelengths; W = 1 with w_step = 0 has w = 0), random
    visibilities and A-terms near the identity, a Kaiser-Bessel taper.
    Returns a dict of arrays; metadata from the host plan."""
    import idg_amd
    o = SMALL
    G, S, C, B, T = o["G"], o["S"], o["C"], o["B"], o["T"]
    rng = np.random.default_rng(seed)
    wn = pc.wavenumbers(C, df=2.0e6)
    lam0 = 2 * np.pi / float(wn[0])
    cells = lam0 / o["image_size"]          # metres per uv cell, channel 0
    uvw = np.zeros((B, T, 3), np.float64)
    for bl in range(B):
        r = rng.uniform(0.08, 0.30) * G
        a0 = rng.uniform(0, 2 * np.pi)
        ang = a0 + rng.uniform(0.2, 0.5) * np.arange(T) / T
        uvw[bl, :, 0] = r * np.cos(ang) * cells
        uvw[bl, :, 1] = 0.8 * r * np.sin(ang) * cells
        if w_step:
            w0 = rng.uniform(0.1, W - 0.1) * w_step
            uvw[bl, :, 2] = (w0 + rng.uniform(-0.3, 0.3) * w_step
                             * np.arange(T) / T) * lam0
    uvw = uvw.astype(F)
    st = 4
    base = np.array([(i, j) for i in range(st) for j in range(i + 1, st)],
                    np.int32)[:B]
    vis = rng.normal(size=(B * T, C, 4, 2)).astype(F)
    at = (0.1 * rng.normal(size=(1, st, S, S, 4, 2))).astype(F)
    at[..., 0, 0] += 1.0
    at[..., 3, 0] += 1.0
    sph = kaiser_taper(S)
    md, dropped = idg_amd.plan(G, S, o["image_size"], w_step, uvw,
                               np.ascontiguousarray(base), wn, o["K"],
                               o["Tmax"], 0, W)
    assert dropped == 0 and md.size >= B
    return dict(uvw=uvw, baselines=base, wn=wn, vis=vis, aterms=at,
                spheroidal=np.ascontiguousarray(sph), md=md, nr_stations=st,
                W=W, w_step=float(w_step))


def correction_for(case, floor=0.05):
    """1 / taper_to_image where the taper exceeds `floor` of its peak, 0
    elsewhere (the part of the field this test images), and that mask."""
    import idg_amd
    t = idg_amd.taper_to_image(SMALL["S"], SMALL["G"],
                               case["spheroidal"]).astype(np.float64)
    mask = t > floor * t.max()
    return np.where(mask, 1.0 / np.where(mask, t, 1.0), 0.0), mask


def identity_aterms(case):
    at = np.zeros_like(case["aterms"])
    at[..., 0, 0] = 1.0
    at[..., 3, 0] = 1.0
    return at


def chain_invert(oracle_lib, case, vis, correction, aterms=None):
    """vis -> oracle gridder -> subgrid FFT (+1) -> adder -> grid_to_image
    with correction / S^2: the image [4, G, G] (complex128)."""
    o, md = case.get("geom", SMALL), case["md"]
    G, S = o["G"], o["S"]
    sg = np.zeros((md.size, 4, S, S, 2), F)
    oracle_lib.gridder(md.size, G, S, o["image_size"], case["w_step"], o["C"],
                       case["nr_stations"], case["uvw"], case["wn"], vis,
                       case["spheroidal"],
                       case["aterms"] if aterms is None else aterms, md, sg)
    grid = pl.adder(np.zeros((case["W"], 4, G, G), complex), md,
                    pl.subgrid_fft(pl.to_complex(sg), +1))
    return grid_to_image(grid, o["image_size"], case["w_step"],
                         correction / (S * S))


def chain_predict(oracle_lib, case, image, correction, aterms=None):
    """image -> image_to_grid -> splitter -> subgrid FFT (-1, 1/S^2) ->
    oracle degridder: visibilities [rows, C, 4] (complex128); rows outside
    every subgrid stay 0."""
    o, md = case.get("geom", SMALL), case["md"]
    G, S = o["G"], o["S"]
    grid = image_to_grid(image, case["W"], o["image_size"], case["w_step"],
                         correction)
    sg = pl.to_pairs(pl.subgrid_fft(pl.splitter(grid, md, S), -1,
                                    1.0 / (S * S)))
    vis = np.zeros_like(case["vis"])
    oracle_lib.degridder(md.size, G, S, o["image_size"], case["w_step"],
                         o["C"], case["nr_stations"], case["uvw"], case["wn"],
                         vis, case["spheroidal"],
                         case["aterms"] if aterms is None else aterms, md,
                         np.ascontiguousarray(sg))
    return pl.to_complex(vis)


def covered_rows(case):
    """Mask over the visibility rows some subgrid covers."""
    rows = np.zeros(case["uvw"].shape[0] * case["uvw"].shape[1], bool)
    for m in case["md"]:
        rows[m["time_offset"]:m["time_offset"] + m["nr_timesteps"]] = True
    return rows


# ---- the contract's direct sums (identity A-terms) -------------------------
def _phase(case):
    """k_c (u l + v m + w n) as [rows, C, G, G] pieces: returns (uvw rows
    [R, 3] float64, wavenumbers [C], l [G], n [G, G])."""
    uvw = case["uvw"].reshape(-1, 3).astype(np.float64)
    o = case.get("geom", SMALL)
    l = lm(o["G"], o["image_size"])
    return uvw, case["wn"].astype(np.float64), l, n_of(l, l)


def direct_invert(case, vis):
    """I[:, y, x] = sum_{row, c} V exp(-i k_c (u l_x + v m_y + w n)) over the
    covered rows, identity A-terms; vis complex [rows, C, 4]."""
    uvw, wn, l, n = _phase(case)
    G = l.size
    image = np.zeros((4, G, G), complex)
    for r in np.flatnonzero(covered_rows(case)):
        geo = uvw[r, 0] * l[None, :] + uvw[r, 1] * l[:, None] + uvw[r, 2] * n
        for c in range(wn.size):
            image += vis[r, c][:, None, None] * np.exp(-1j * wn[c] * geo)
    return image


def direct_predict(case, image):
    """V(row, c) = sum_{y, x} I[:, y, x] exp(+i k_c (u l_x + v m_y + w n)),
    identity A-terms; complex [rows, C, 4], uncovered rows 0."""
    uvw, wn, l, n = _phase(case)
    vis = np.zeros((uvw.shape[0], wn.size, 4), complex)
    ys, xs = np.nonzero(np.abs(image).sum(axis=0))
    for r in np.flatnonzero(covered_rows(case)):
        geo = uvw[r, 0] * l[xs] + uvw[r, 1] * l[ys] + uvw[r, 2] * n[ys, xs]
        for c in range(wn.size):
            vis[r, c] = image[:, ys, xs] @ np.exp(1j * wn[c] * geo)
    return vis
