"""Debug aid (CPU): the ordered gridder (IDG_GRIDDER_IMPL=ordered, csrc/hip/
kernels/ordered_mi355x.hip.cpp) emulated in exact f32 numpy: the reference's
summation order (t, then c, pixel += visibility * phasor in product form b,
two f32 adds) with the phasor taken from one of

  cr    correctly rounded f32 sin / cos of the reference's f32 phase
  rev   r = revolutions(phase) (device.hpp, emulated exactly), then correctly
        rounded f32 sin / cos of 2 pi r            -- deterministic
  hw    rev plus uniform noise of +-HW (default 1.25e-7: hw_small of
        profiles/r01/sincos_probe.txt taken as the amplitude, about twice the
        measured rms) on each output: a model of v_sin_f32 / v_cos_f32

and the epilogue (A1^H P A2, taper) in f64, scored in the reference metric
against the oracle (bit-exact to the reference's CPU output).  Products of
two floats are exact in float64, so fma32(a, b, c) = f32(a * b + c) is the
device's fmaf (tools/debug/tail_emul.py).

    python tests/emul/ordered_emul.py [C] [T] [variant ...]
DESIGN.md §3.5.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in ("ska-sdp-idg-bench_amd", "oracle"):
    if os.path.join(REPO, _p) not in sys.path:
        sys.path.insert(0, os.path.join(REPO, _p))

f32, f64 = np.float32, np.float64
IH = f32(float.fromhex("0x1.45f306p-3"))      # device.hpp kInv2PiHi
IH_LO = f32(float.fromhex("0x1.b9391p-28"))   # device.hpp kInv2PiLo
VARIANTS = ("cr", "rev", "hw")


def fma32(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def revolutions(x):
    """device.hpp revolutions(): Dekker head product, tail, round to nearest."""
    hi = (x * IH).astype(f32)
    lo = fma32(x, IH, -hi)
    lo = fma32(x, IH_LO, lo)
    return ((hi - np.rint(hi)).astype(f32) + lo).astype(f32)


def phasor(ph, variant, hw, rng):
    """(sin, cos) in f32 of the f32 phases ph."""
    if variant == "cr":
        ang = ph.astype(f64)
    else:
        ang = 2.0 * np.pi * revolutions(ph).astype(f64)
    sn, cs = np.sin(ang), np.cos(ang)
    if variant == "hw":
        sn = sn + rng.uniform(-hw, hw, sn.shape)
        cs = cs + rng.uniform(-hw, hw, cs.shape)
    return sn.astype(f32), cs.astype(f32)


def geometry(S, G, image_size, w_step, md):
    """l, m, n, phase_offset of every pixel as the reference gridder forms
    them (csrc/common/math.hpp, device.hpp setup_subgrid)."""
    img = f32(image_size)
    idx = ((np.arange(S) + 0.5 - S // 2) * f64(img) / S).astype(f32)
    l = np.broadcast_to(idx[None, :], (S, S)).astype(f32).ravel()
    m = np.broadcast_to(idx[:, None], (S, S)).astype(f32).ravel()
    tmp = fma32(l, l, (m * m).astype(f32))
    with np.errstate(invalid="ignore"):
        n = np.where(tmp > 1, f32(1), tmp / (f32(1) + np.sqrt(f32(1) - tmp))).astype(f32)
    scale = 2.0 * np.pi / f64(img)
    uo = f32((int(md["x"]) + S // 2 - G // 2) * scale)
    vo = f32((int(md["y"]) + S // 2 - G // 2) * scale)
    wl = f32(f64(f32(w_step)) * (f64(int(md["z"])) + 0.5))
    wo = f32(2.0 * np.pi * f64(wl))
    poff = fma32(wo, n, fma32(uo, l, (vo * m).astype(f32)))
    return l, m, n, poff


def emulate_subgrid(a, s, G, S, image_size, w_step, nr_stations, variant,
                    hw=1.25e-7, seed=0):
    """Subgrid s of the arrays `a` (idg_amd.generate layout) as the ordered
    gridder computes it: [4][S][S][2] float32."""
    rng = np.random.default_rng(seed)
    md = a["metadata"][s]
    C = a["wavenumbers"].size
    k = a["wavenumbers"].astype(f32)
    npix = S * S
    l, m, n, poff = geometry(S, G, image_size, w_step, md)
    T = int(md["nr_timesteps"])
    row0 = int(md["baseline_offset"] - a["metadata"][0]["baseline_offset"]) + \
        int(md["time_offset"])
    uvw = a["uvw"].reshape(-1, 3)[row0:row0 + T]
    vis = a["visibilities"].reshape(-1, C, 4, 2)[row0:row0 + T]
    # acc rows 0-3: re of the 4 correlations, rows 4-7: im
    acc = np.zeros((8, npix), f32)
    for t in range(T):
        u, v, w = uvw[t]
        pidx = fma32(w, n, fma32(u, l, (v * m).astype(f32)))
        ph = fma32(-pidx[None, :], k[:, None], poff[None, :])    # [C][npix]
        sn, cs = phasor(ph, variant, hw, rng)
        vr, vi = vis[t, :, :, 0], vis[t, :, :, 1]                # [C][4]
        a8 = np.concatenate([vr, vi], 1).astype(f64)[:, :, None]  # (vr, vi)
        b8 = np.concatenate([-vi, vr], 1)[:, :, None]             # (-vi, vr)
        for c in range(C):
            # re = fma(vr, c, -(vi * s)), im = fma(vi, c, vr * s): form b
            t8 = b8[c] * sn[c][None, :]                           # f32 product
            acc += (a8[c] * cs[c][None, :].astype(f64) + t8).astype(f32)
    P = (acc[:4].astype(f64) + 1j * acc[4:]).T.reshape(S, S, 2, 2)
    at = a["aterms"].reshape(-1, nr_stations, S, S, 4, 2)
    at = at[..., 0].astype(f64) + 1j * at[..., 1]
    a1 = at[int(md["aterm_index"]), int(md["station1"])].reshape(S, S, 2, 2)
    a2 = at[int(md["aterm_index"]), int(md["station2"])].reshape(S, S, 2, 2)
    P = np.conj(np.swapaxes(a1, -1, -2)) @ P @ a2
    P = P.reshape(S, S, 4) * a["spheroidal"].astype(f64)[..., None]
    out = np.empty((4, S, S, 2), f32)
    out[..., 0] = np.moveaxis(P.real, -1, 0)
    out[..., 1] = np.moveaxis(P.imag, -1, 0)
    return out


def distances(T, C, variant, subgrids=(0, 1), st=2, ts=2, G=1024, S=32,
              hw=1.25e-7, nthreads=4):
    """Reference-metric distance of the emulated ordered gridder to the
    oracle, per subgrid of idg_amd.generate(st, ts, T, C, G, S)."""
    import idg_amd
    import oracle as orc
    o = orc.Oracle()
    a = idg_amd.generate(st, ts, T, C, G, S, nthreads=nthreads)
    ns = a["metadata"].size
    go = np.zeros((ns, 4, S, S, 2), f32)
    o.gridder(ns, G, S, idg_amd.IMAGE_SIZE, 0.0, C, st, a["uvw"],
              a["wavenumbers"], a["visibilities"], a["spheroidal"],
              a["aterms"], a["metadata"], go, nthreads=nthreads)
    return [o.check_error(emulate_subgrid(a, s, G, S, idg_amd.IMAGE_SIZE, 0.0,
                                          st, variant, hw, seed=s)[None],
                          go[s:s + 1])[0] for s in subgrids]


if __name__ == "__main__":
    C = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    for variant in sys.argv[3:] or VARIANTS:
        d = distances(T, C, variant)
        print(f"T={T} C={C} {variant:4s} " + " ".join(f"{x:.3e}" for x in d))
