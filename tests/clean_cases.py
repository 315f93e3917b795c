"""The Hogbom minor cycle's contract (include/idg_mi355x.h)
restated in numpy, and the seeded cases of test_clean_host.py (host entry
against this restatement) and test_gpu_clean.py (device entry against the host
entry).  Everything is float32; every operation below rounds once."""
import numpy as np

F = np.float32
COMPONENT = np.dtype([("y", "<i4"), ("x", "<i4"), ("value", "<f4")])
STATE = np.dtype([("n_components", "<i4"), ("reason", "<i4"),
                  ("started", "<i4"), ("peak_index", "<i4"),
                  ("level", "<f4"), ("peak", "<f4")])
GUARD = F(-12345.678)
GUARD_INT = -0x1234567


# ---- the contract ------------------------------------------------------------
def fmaf(a, b, c):
    """fmaf(a, b, c) of float32 arrays: a * b + c rounded once.

    np.float32 has no fused multiply-add.  The product of two float32 (24-bit
    significands) has at most 48 bits and is exact in float64 (53).  The sum
    with c is then rounded to float64 and again to float32.  Two roundings
    differ from one only when the float64 sum lands exactly half-way between
    two float32 while the exact sum does not: that needs an exact sum of more
    than 53 bits, so the product and c far apart in exponent and a tail of
    about 29 particular bits -- for c and the product within 2^5 of each other
    it cannot happen at all.  The few lines after the sum close that gap: the
    exact error of the float64 sum (Knuth's TwoSum) says on which side of the
    half-way point the exact sum lies, and the float64 is moved one step
    there before it is rounded to float32.  test_clean_host.py checks this
    function against the host entry's own subtraction on 10^6 random triples.
    (Results in float32's normal range; the cases stay there.)"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        tie = (s.view(np.uint64) & np.uint64(0x1fffffff)) == np.uint64(
            0x10000000)
        move = tie & np.isfinite(err) & (err != 0)
        s = np.where(move, np.nextafter(s, np.where(err > 0, np.inf,
                                                    -np.inf)), s)
        return s.astype(F)


def peak(residual, mask):
    """Linear index of the largest |s| among the searchable, non-NaN pixels,
    the lowest index among equals (+v and -v too); -1 if there is none."""
    a = np.abs(residual).ravel()
    ok = ~np.isnan(a)
    if mask is not None:
        ok &= mask.ravel() != 0
    if not ok.any():
        return -1
    return int(np.argmax(np.where(ok, a, F(-1))))   # argmax: first of equals


def restate(residual, psf, model, mask, components, state, gain, threshold,
            cycle_fraction, max_components, nr_iterations):
    """One call of the contract on numpy buffers, in place, continuing from
    `state` (STATE [1])."""
    G, Gp = residual.shape[0], psf.shape[0]
    gain, threshold, cycle_fraction = F(gain), F(threshold), F(cycle_fraction)
    st = state[0]
    for _ in range(nr_iterations):
        if st["reason"] != 0:
            break
        i = peak(residual, mask)
        if i < 0:
            st["reason"] = 2
            break
        py, px = divmod(i, G)
        v = residual[py, px]
        a = np.abs(v)
        if st["started"] == 0:
            st["level"] = np.fmax(threshold, F(cycle_fraction * a))
            st["started"] = 1
        if not a > st["level"]:
            st["reason"] = 1
            break
        n = int(st["n_components"])
        if n == max_components:
            st["reason"] = 3
            break
        c = F(gain * v)
        components[n] = (py, px, c)
        st["n_components"] = n + 1
        model[py, px] = F(model[py, px] + c)
        oy, ox = py - Gp // 2, px - Gp // 2
        y0, y1 = max(oy, 0), min(oy + Gp, G)
        x0, x1 = max(ox, 0), min(ox + Gp, G)
        cut = residual[y0:y1, x0:x1]
        cut[...] = fmaf(np.full(cut.shape, -c, F),
                        psf[y0 - oy:y1 - oy, x0 - ox:x1 - ox], cut)
    i = peak(residual, mask)
    st["peak"] = np.abs(residual.ravel()[i]) if i >= 0 else F(0)
    st["peak_index"] = i


# ---- seeded inputs -----------------------------------------------------------
def psf_plane(Gp, seed=1):
    """A seeded random plane, |sidelobes| <= 0.3, centre 1."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.3, 0.3, (Gp, Gp)).astype(F)
    p[Gp // 2, Gp // 2] = 1.0
    return p


def residual_plane(G, psf, sources, noise=0.01, seed=2):
    """Point sources (y, x, flux) convolved with the PSF by hand, plus
    noise."""
    rng = np.random.default_rng(seed)
    Gp = psf.shape[0]
    r = (noise * rng.normal(size=(G, G))).astype(F)
    for y, x, flux in sources:
        oy, ox = y - Gp // 2, x - Gp // 2
        y0, y1, x0, x1 = max(oy, 0), min(oy + Gp, G), max(ox, 0), min(
            ox + Gp, G)
        r[y0:y1, x0:x1] += F(flux) * psf[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    return r


def case(G, Gp, sources, chunks=(8,), gain=0.2, threshold=0.0,
         cycle_fraction=0.0, max_components=None, mask=None, model=None,
         noise=0.01, seed=2, edit=None):
    psf = psf_plane(Gp, seed + 100)
    residual = residual_plane(G, psf, sources, noise, seed)
    if edit is not None:
        edit(residual)
    total = sum(chunks)
    return dict(G=G, Gp=Gp, residual=residual, psf=psf, mask=mask,
                model=model, chunks=tuple(chunks), gain=gain,
                threshold=threshold, cycle_fraction=cycle_fraction,
                max_components=total if max_components is None
                else max_components)


def _set(*pixels):
    def edit(r):
        for y, x, v in pixels:
            r[y, x] = v
    return edit


def _mask_hiding(G, y, x, reach=3):
    m = np.ones((G, G), np.uint8)
    m[max(y - reach, 0):y + reach + 1, max(x - reach, 0):x + reach + 1] = 0
    return m


def _start_model(G, seed=9):
    return np.random.default_rng(seed).normal(size=(G, G)).astype(F)


THREE = [(11, 27, 5.0), (30, 8, -3.0), (20, 20, 2.0)]

CASES = {
    "G40_Gp40": lambda: case(40, 40, THREE, chunks=(25,)),
    "G65_Gp16_odd_G": lambda: case(65, 16, [(5, 60, 4.0), (40, 33, 3.0),
                                            (64, 2, -2.5)], chunks=(20,)),
    "G33_Gp7_odd_Gp": lambda: case(33, 7, [(16, 16, 3.0), (2, 30, 2.0)],
                                   chunks=(20,)),
    "peak_at_0_0": lambda: case(40, 16, [(0, 0, 6.0), (25, 25, 1.0)],
                                chunks=(6,)),
    "peak_at_last": lambda: case(40, 16, [(39, 39, 6.0), (10, 10, 1.0)],
                                 chunks=(6,)),
    "tie_lower_index_wins": lambda: case(
        40, 8, [], chunks=(4,), edit=_set((10, 30, 7.0), (25, 5, 7.0))),
    "tie_plus_minus": lambda: case(
        40, 8, [], chunks=(4,), edit=_set((8, 8, -7.0), (20, 3, 7.0))),
    "negative_peak": lambda: case(40, 16, [(12, 14, -5.0)], chunks=(6,)),
    "nan_pixel": lambda: case(
        40, 7, [(10, 10, 4.0), (15, 20, 3.0)], chunks=(10,),
        edit=_set((30, 30, np.nan))),
    "mask_hides_the_maximum": lambda: case(
        40, 16, THREE, chunks=(10,), mask=_mask_hiding(40, 11, 27)),
    "mask_all_zero": lambda: case(
        40, 16, THREE, chunks=(5,), mask=np.zeros((40, 40), np.uint8)),
    "threshold_reached": lambda: case(
        40, 16, [(20, 21, 10.0)], chunks=(25,), gain=0.5, threshold=1.0,
        noise=0.001),
    "cycle_fraction": lambda: case(
        40, 16, [(20, 21, 10.0), (5, 7, 6.0)], chunks=(25,), gain=0.3,
        cycle_fraction=0.5),
    "components_full": lambda: case(40, 16, THREE, chunks=(10,),
                                    max_components=4),
    "zero_iterations": lambda: case(40, 16, THREE, chunks=(0,),
                                    max_components=5),
    "three_calls_of_5": lambda: case(40, 16, THREE, chunks=(5, 5, 5)),
    "one_call_of_15": lambda: case(40, 16, THREE, chunks=(15,)),
    "model_accumulates": lambda: case(
        40, 16, [(17, 9, 8.0)], chunks=(6,), gain=0.2,
        model=_start_model(40)),
    "all_zero_residual": lambda: case(
        40, 16, [], chunks=(5,), noise=0.0),
}


# Shapes for the device's tiles (256 columns x 8 rows up to G = 2048): several
# tiles, whose carried-forward partials must still be right when a later patch
# lands on them; and at G = 2048 more partials (2048) than a workgroup has
# threads, with peaks in the first tile, in the last one and on the corner
# where four tiles meet.
# (fluxes a factor 0.8 = 1 - gain apart or less, so that the peak moves from
# source to source and comes back)
FIVE = [(20, 200, 6.0), (130, 7, -5.6), (250, 250, 5.2), (100, 128, 4.8),
        (7, 3, 4.4)]
LARGE = {
    "G256_Gp256": lambda: case(256, 256, FIVE, chunks=(40,)),
    "G256_Gp32": lambda: case(256, 32, FIVE, chunks=(40,)),
    "G2048_Gp64": lambda: case(
        2048, 64, [(3, 100, 9.0), (2047, 2040, -8.0), (8, 256, 7.0)],
        chunks=(8,), gain=0.5),
}


# ---- guarded buffers and runs --------------------------------------------------
def buffers(c):
    """residual and model between two guard rows, components between two guard
    records, a zeroed state: numpy, the whole allocations."""
    G, M = c["G"], max(c["max_components"], 1)
    residual = np.full((G + 2, G), GUARD, F)
    residual[1:-1] = c["residual"]
    model = np.full((G + 2, G), GUARD, F)
    model[1:-1] = 0 if c["model"] is None else c["model"]
    components = np.zeros(M + 2, COMPONENT)
    components[[0, -1]] = (GUARD_INT, GUARD_INT, GUARD)
    return dict(residual=residual, model=model, components=components,
                state=np.zeros(1, STATE))


def guards_intact(b):
    g = np.array([(GUARD_INT, GUARD_INT, GUARD)], COMPONENT)
    return (np.all(b["residual"][[0, -1]] == GUARD)
            and np.all(b["model"][[0, -1]] == GUARD)
            and b["components"][0] == g[0] and b["components"][-1] == g[0])


def params(c):
    return dict(gain=c["gain"], threshold=c["threshold"],
                cycle_fraction=c["cycle_fraction"],
                max_components=c["max_components"])


def run_restatement(c):
    """The case through restate(), chunk by chunk; the buffers() it leaves."""
    b = buffers(c)
    for n in c["chunks"]:
        restate(b["residual"][1:-1], c["psf"], b["model"][1:-1], c["mask"],
                b["components"][1:-1], b["state"], nr_iterations=n,
                **params(c))
    return b


def run_host(idg, c):
    """The case through the host entry, chunk by chunk; the buffers()."""
    b = buffers(c)
    for n in c["chunks"]:
        idg.clean(b["residual"][1:-1], c["psf"], b["model"][1:-1], c["mask"],
                  nr_iterations=n, components=b["components"][1:-1],
                  state=b["state"], **params(c))
    return b


def same_bytes(a, b):
    """Names of the buffers() entries whose bytes differ."""
    return [k for k in a if a[k].tobytes() != b[k].tobytes()]
