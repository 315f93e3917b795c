"""Multi-scale CLEAN's contract (include/idg_mi355x.h) restated
in numpy, and the seeded cases of test_multiscale_host.py (host entries against
this restatement) and test_gpu_multiscale.py (device entries against the host
entries).  Everything but the taps is float32; every operation rounds once."""
import numpy as np

from clean_cases import F, GUARD, GUARD_INT, fmaf

COMPONENT = np.dtype([("y", "<i4"), ("x", "<i4"), ("scale", "<i4"),
                      ("value", "<f4")])
STATE = np.dtype([("n_components", "<i4"), ("reason", "<i4"),
                  ("started", "<i4"), ("peak_index", "<i4"),
                  ("level", "<f4"), ("peak", "<f4"), ("peak_scale", "<i4")])


# ---- the contract ------------------------------------------------------------
def scale_radius(a):
    return 0 if a == 0 else int(np.ceil(3.0 * (a * 3.0 / 16.0)))


def scale_taps64(a):
    """A scale's taps before the rounding to float32, in float64."""
    if a == 0:
        return np.ones(1)
    sigma = a * 3.0 / 16.0
    r = scale_radius(a)
    e = [np.exp(-float(k * k) / (2.0 * sigma * sigma))
         for k in range(-r, r + 1)]
    total = 0.0
    for v in e:
        total += v
    return np.array(e) / total


def convolve(image, taps):
    """The row pass, then the column pass; (tmp, out)."""
    G, r = image.shape[0], taps.size // 2

    def one_pass(src):
        acc = np.zeros((G, G), F)
        for k in range(-r, r + 1):
            a, b = max(0, -k), min(G, G - k)      # x with 0 <= x + k < G
            if a < b:
                acc[:, a:b] = fmaf(src[:, a + k:b + k],
                                   np.full((G, b - a), taps[k + r], F),
                                   acc[:, a:b])
        return acc
    tmp = one_pass(image)
    return tmp, np.ascontiguousarray(one_pass(np.ascontiguousarray(tmp.T)).T)


def cross_at(Ns, s, q):
    lo, hi = min(s, q), max(s, q)
    return lo * Ns - lo * (lo - 1) // 2 + (hi - lo)


def prepare(residual, psf, taps):
    """(planes [Ns][G][G], cross_psf [Ns (Ns + 1) / 2][Gp][Gp])."""
    Ns = len(taps)
    planes = np.stack([residual] + [convolve(residual, h)[1]
                                    for h in taps[1:]])
    cross = np.zeros((Ns * (Ns + 1) // 2,) + psf.shape, F)
    for s in range(Ns):
        first = convolve(psf, taps[s])[1]
        for q in range(s, Ns):
            cross[cross_at(Ns, s, q)] = convolve(first, taps[q])[1]
    return planes, cross


def weights(cross, scales, scale_bias=0.6):
    """The default (weight, inv_peak), in doubles, rounded once."""
    Ns, Gp = len(scales), cross.shape[-1]
    inv = np.array([1.0 / float(cross[cross_at(Ns, s, s), Gp // 2, Gp // 2])
                    for s in range(Ns)])
    a_max = max(scales)
    bias = np.array([1.0 if a_max == 0 else 1.0 - scale_bias * a / a_max
                     for a in scales])
    return (bias * inv).astype(F), inv.astype(F)


def peak(planes, weight, mask):
    """(scale, linear index) of the largest |weight[s] * v| among the
    searchable pixels with neither v nor the product NaN: the lowest scale,
    then the lowest index among equals; (-1, -1) if there is none."""
    Ns = planes.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.abs(planes * np.asarray(weight, F)[:, None, None]).reshape(Ns, -1)
    ok = ~np.isnan(u)
    if mask is not None:
        ok &= (mask.ravel() != 0)[None, :]
    if not ok.any():
        return -1, -1
    at = int(np.argmax(np.where(ok, u, F(-1))))      # first of equals
    return divmod(at, u.shape[1])


def restate(planes, cross, taps, weight, inv_peak, mask, model, components,
            state, gain, threshold, cycle_fraction, max_components,
            nr_iterations):
    """One call of the minor cycle on numpy buffers, in place, continuing
    from `state` (STATE [1])."""
    Ns, G, Gp = planes.shape[0], planes.shape[1], cross.shape[1]
    gain, threshold, cycle_fraction = F(gain), F(threshold), F(cycle_fraction)
    weight, inv_peak = np.asarray(weight, F), np.asarray(inv_peak, F)
    st = state[0]
    for _ in range(nr_iterations):
        if st["reason"] != 0:
            break
        s, i = peak(planes, weight, mask)
        if i < 0:
            st["reason"] = 2
            break
        py, px = divmod(i, G)
        v = planes[s, py, px]
        u = np.abs(F(weight[s] * v))
        if st["started"] == 0:
            st["level"] = np.fmax(threshold, F(cycle_fraction * u))
            st["started"] = 1
        if not u > st["level"]:
            st["reason"] = 1
            break
        n = int(st["n_components"])
        if n == max_components:
            st["reason"] = 3
            break
        c = F(F(gain * v) * inv_peak[s])
        components[n] = (py, px, s, c)
        st["n_components"] = n + 1
        h, r = taps[s], taps[s].size // 2
        y0, y1 = max(py - r, 0), min(py + r + 1, G)
        x0, x1 = max(px - r, 0), min(px + r + 1, G)
        hy = h[y0 - py + r:y1 - py + r][:, None]
        hx = h[x0 - px + r:x1 - px + r][None, :]
        model[y0:y1, x0:x1] = (model[y0:y1, x0:x1] +
                               (F(c) * hy).astype(F) * hx).astype(F)
        oy, ox = py - Gp // 2, px - Gp // 2
        y0, y1 = max(oy, 0), min(oy + Gp, G)
        x0, x1 = max(ox, 0), min(ox + Gp, G)
        for q in range(Ns):
            cut = planes[q, y0:y1, x0:x1]
            cut[...] = fmaf(np.full(cut.shape, -c, F),
                            cross[cross_at(Ns, s, q), y0 - oy:y1 - oy,
                                  x0 - ox:x1 - ox], cut)
    s, i = peak(planes, weight, mask)
    if i >= 0:
        st["peak"] = np.abs(F(weight[s] * planes[s].ravel()[i]))
    else:
        st["peak"] = F(0)
    st["peak_index"], st["peak_scale"] = i, s


# ---- guarded buffers -----------------------------------------------------------
def guarded(a):
    """`a` ([..., n, n]) between two guard rows of n: the whole allocation."""
    n = a.shape[-1]
    g = np.full((a.size // n + 2, n), GUARD, F)
    g[1:-1] = a.reshape(-1, n)
    return g


def inner(g, shape):
    return g[1:-1].reshape(shape)


def guards_ok(g):
    return bool(np.all(g[[0, -1]].view(np.uint32)
                       == np.array(GUARD, F).view(np.uint32)))


def guarded_components(n):
    c = np.zeros(max(n, 1) + 2, COMPONENT)
    c[[0, -1]] = (GUARD_INT, GUARD_INT, GUARD_INT, GUARD)
    return c


def component_guards_ok(c):
    g = np.array([(GUARD_INT, GUARD_INT, GUARD_INT, GUARD)], COMPONENT)
    return bool(c[0] == g[0] and c[-1] == g[0])


# ---- convolution cases -----------------------------------------------------------
# scale -> radius: 4 -> 3, 16 -> 9, 85 -> 48 (the largest allowed)
def _random(G, seed):
    return np.random.default_rng(seed).normal(size=(G, G)).astype(F)


def _deltas(G, at):
    a = np.zeros((G, G), F)
    for n, (y, x) in enumerate(at):
        a[y, x] = F(1.0 + 0.25 * n)
    return a


def _nonfinite(G, seed):
    a = _random(G, seed)
    a[G // 3, G // 2] = np.nan
    a[G - 2, 1] = np.inf
    return a


# the device's tiles: the row pass 256 columns x 8 rows, the column pass 64
# columns x 64 rows: seams at columns 63/64, 255/256 and rows 7/8, 63/64
SEAMS = [(0, 0), (0, 259), (259, 0), (259, 259), (7, 255), (8, 256),
         (63, 63), (64, 64), (130, 255), (131, 256), (200, 127), (201, 128)]

CONV = {
    "G8_r9_wider_than_the_image": lambda: (_random(8, 1), 16),
    "G5_r0": lambda: (_random(5, 2), 0),
    "G258_r3_scalar": lambda: (_random(258, 3), 4),
    "G260_r3_vector": lambda: (_random(260, 4), 4),
    "G260_r48_vector": lambda: (_random(260, 5), 85),
    "G258_r48_scalar": lambda: (_random(258, 6), 85),
    "G36_nan_and_inf": lambda: (_nonfinite(36, 7), 8),
    "G260_deltas_r3": lambda: (_deltas(260, SEAMS), 4),
    "G260_deltas_r9": lambda: (_deltas(260, SEAMS), 16),
}


# ---- prepare and minor-cycle cases ----------------------------------------------
def psf_plane(Gp, seed=1):
    """A main lobe of sigma 1.2 plus seeded sidelobes of at most 0.1, centre
    1."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:Gp, :Gp] - Gp // 2
    p = (np.exp(-(y * y + x * x) / (2 * 1.2 ** 2))
         + rng.uniform(-0.1, 0.1, (Gp, Gp)))
    p[Gp // 2, Gp // 2] = 1.0
    return p.astype(F)


def dirty_plane(G, psf, blobs, noise=0.01, seed=2):
    """Gaussian blobs (y, x, flux at the centre, sigma; sigma 0: a point)
    convolved with the PSF by hand, plus noise."""
    rng = np.random.default_rng(seed)
    Gp = psf.shape[0]
    yy, xx = np.mgrid[:G, :G]
    sky = np.zeros((G, G))
    for y, x, flux, sigma in blobs:
        if sigma == 0:
            sky[y, x] += flux
        else:
            sky += flux * np.exp(-((yy - y) ** 2 + (xx - x) ** 2)
                                 / (2.0 * sigma ** 2))
    sky[np.abs(sky) < 1e-3] = 0
    r = noise * rng.normal(size=(G, G))
    for y, x in zip(*np.nonzero(sky)):
        oy, ox = y - Gp // 2, x - Gp // 2
        y0, y1, x0, x1 = max(oy, 0), min(oy + Gp, G), max(ox, 0), min(
            ox + Gp, G)
        r[y0:y1, x0:x1] += sky[y, x] * psf[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    return r.astype(F)


PREP = {
    "G64_Gp33_scales_0_4_8": lambda: dict(
        G=64, Gp=33, scales=(0, 4, 8),
        blobs=[(20, 40, 1.0, 3.0), (50, 10, 3.0, 0)]),
    "G8_Gp5_scale_16_wider_than_the_psf": lambda: dict(
        G=8, Gp=5, scales=(0, 16), blobs=[(3, 4, 2.0, 0), (7, 0, 1.0, 0)]),
}


def prep_inputs(c, idg):
    """(residual, psf, the library's taps) of a PREP or MS case."""
    psf = psf_plane(c["Gp"], c.get("seed", 2) + 100)
    residual = dirty_plane(c["G"], psf, c["blobs"], c.get("noise", 0.01),
                           c.get("seed", 2))
    return residual, psf, idg.ms_scale_taps(c["scales"])


def ms_case(G, Gp, scales, blobs, chunks=(8,), gain=0.2, threshold=0.0,
            cycle_fraction=0.0, max_components=None, mask=None, edit=None,
            unit_weight=False, noise=0.01, seed=2):
    return dict(G=G, Gp=Gp, scales=tuple(scales), blobs=blobs,
                chunks=tuple(chunks), gain=gain, threshold=threshold,
                cycle_fraction=cycle_fraction,
                max_components=sum(chunks) if max_components is None
                else max_components, mask=mask, edit=edit,
                unit_weight=unit_weight, noise=noise, seed=seed)


def _set(*pixels):
    def edit(planes):
        for s, y, x, v in pixels:
            planes[s, y, x] = v
    return edit


def _mask_hiding(G, y, x, reach=6):
    m = np.ones((G, G), np.uint8)
    m[max(y - reach, 0):y + reach + 1, max(x - reach, 0):x + reach + 1] = 0
    return m


CORNERS = [(0, 0, 5.0, 0), (7, 7, 4.2, 0), (0, 5, -3.6, 0), (4, 7, 3.0, 0)]
EDGES = [(2, 30, 1.0, 4.0), (61, 3, 0.8, 2.5), (30, 62, 4.0, 0),
         (40, 30, 1.2, 1.5)]
TWO = [(30, 34, 1.0, 3.0), (12, 50, 3.0, 0)]

MS = {
    "G8_Gp5_border_and_corners": lambda: ms_case(
        8, 5, (0, 4), CORNERS, chunks=(10,)),
    "G64_Gp33_four_scales_clipped": lambda: ms_case(
        64, 33, (0, 4, 8, 16), EDGES, chunks=(16,)),
    # components of scales 1 and 2 on the column-256 seam and the row-8 seam of
    # the device's tiles (256 columns x 8 rows), and of scale 1 on column 255
    "G260_Gp65_footprint_across_tiles": lambda: ms_case(
        260, 65, (0, 4, 8), [(8, 256, 3.0, 1.5), (135, 255, -4.0, 0.75)],
        chunks=(6,), gain=0.5),
    # G % 4 == 2: the device's one-pixel-per-lane form on planes of its own
    # (every other case has G % 4 == 0).  The host entry takes components of
    # scale 2 at the blob and of scale 0 at the point, in turns.
    "G66_Gp33_scalar_form": lambda: ms_case(
        66, 33, (0, 4, 8), [(20, 41, 0.3, 3.0), (50, 11, 3.0, 0)],
        chunks=(3, 4)),
    "tie_between_scales_lower_scale_wins": lambda: ms_case(
        64, 9, (0, 4), [], chunks=(3,), unit_weight=True,
        edit=_set((1, 10, 30, 7.0), (0, 25, 5, 7.0))),
    "tie_within_a_scale_lower_index_wins": lambda: ms_case(
        64, 9, (0, 4), [], chunks=(3,), unit_weight=True,
        edit=_set((1, 8, 8, -7.0), (1, 20, 3, 7.0))),
    "nan_on_one_scale_only": lambda: ms_case(
        64, 9, (0, 4, 8), TWO, chunks=(8,),
        edit=_set((1, 30, 30, np.nan))),
    "mask_hides_the_maximum": lambda: ms_case(
        64, 33, (0, 4, 8), TWO, chunks=(8,), mask=_mask_hiding(64, 30, 34)),
    "stop_no_peak_mask_all_zero": lambda: ms_case(
        64, 33, (0, 4), TWO, chunks=(4,), mask=np.zeros((64, 64), np.uint8)),
    "stop_below_level": lambda: ms_case(
        64, 33, (0, 4, 8), TWO, chunks=(60,), gain=0.5, threshold=1.0,
        noise=0.001),
    "stop_cycle_fraction": lambda: ms_case(
        64, 33, (0, 4, 8), TWO, chunks=(60,), gain=0.4, cycle_fraction=0.5),
    "stop_components_full": lambda: ms_case(
        64, 33, (0, 4, 8), TWO, chunks=(9,), max_components=4),
    "still_running": lambda: ms_case(64, 33, (0, 4, 8), TWO, chunks=(5,)),
    "zero_iterations": lambda: ms_case(
        64, 33, (0, 4, 8), TWO, chunks=(0,), max_components=5),
    "chunks_3_4_5": lambda: ms_case(64, 33, (0, 4, 8), TWO, chunks=(3, 4, 5)),
    "one_call_of_12": lambda: ms_case(64, 33, (0, 4, 8), TWO, chunks=(12,)),
}


def ms_inputs(c, idg):
    """The minor cycle's inputs of an MS case: planes and cross-PSFs from the
    restatement's prepare on the library's taps, then the case's edits."""
    residual, psf, taps = prep_inputs(c, idg)
    planes, cross = prepare(residual, psf, taps)
    if c["edit"] is not None:
        c["edit"](planes)
    weight, inv_peak = weights(cross, c["scales"])
    if c["unit_weight"]:
        weight = np.ones(len(taps), F)
    return dict(planes=planes, cross=cross, taps=taps, weight=weight,
                inv_peak=inv_peak)


def ms_buffers(c, i):
    G = c["G"]
    return dict(planes=guarded(i["planes"]),
                model=guarded(np.zeros((G, G), F)),
                components=guarded_components(c["max_components"]),
                state=np.zeros(1, STATE))


def ms_params(c):
    return dict(gain=c["gain"], threshold=c["threshold"],
                cycle_fraction=c["cycle_fraction"],
                max_components=c["max_components"])


def ms_guards_ok(b):
    return (guards_ok(b["planes"]) and guards_ok(b["model"])
            and component_guards_ok(b["components"]))


def run_restatement(c, i):
    b = ms_buffers(c, i)
    Ns, G = len(c["scales"]), c["G"]
    for n in c["chunks"]:
        restate(inner(b["planes"], (Ns, G, G)), i["cross"], i["taps"],
                i["weight"], i["inv_peak"], c["mask"],
                inner(b["model"], (G, G)), b["components"][1:-1], b["state"],
                nr_iterations=n, **ms_params(c))
    return b


def run_host(idg, c, i):
    b = ms_buffers(c, i)
    Ns, G = len(c["scales"]), c["G"]
    for n in c["chunks"]:
        idg.ms_clean(inner(b["planes"], (Ns, G, G)), i["cross"], i["taps"],
                     i["weight"], i["inv_peak"],
                     model=inner(b["model"], (G, G)), mask=c["mask"],
                     nr_iterations=n, components=b["components"][1:-1],
                     state=b["state"], **ms_params(c))
    return b


def same_bytes(a, b):
    """Names of the entries whose bytes differ."""
    return [k for k in a if a[k].tobytes() != b[k].tobytes()]


# ---- the property case -----------------------------------------------------------
def property_field():
    """(dirty [64][64], psf [63][63]): a Gaussian blob of sigma 5 and peak 1
    at (30, 34) plus a point of 3.0 at (12, 50), convolved by hand (float64,
    every sky pixel above 1e-3) with a PSF that has a sigma = 1.2 main lobe
    and damped cosine sidelobes, centre 1.  No noise."""
    G, Gp = 64, 63
    y, x = np.mgrid[:Gp, :Gp] - Gp // 2
    rho = np.hypot(y, x)
    lobe = np.exp(-rho ** 2 / (2 * 1.2 ** 2))
    psf = lobe + 0.05 * np.cos(0.9 * rho) * np.exp(-rho / 10.0) * (1 - lobe)
    psf = psf.astype(F)
    assert psf[Gp // 2, Gp // 2] == 1
    dirty = dirty_plane(G, psf, [(30, 34, 1.0, 5.0), (12, 50, 3.0, 0)],
                        noise=0.0)
    return dirty, psf


PROPERTY = dict(gain=0.1, threshold=0.3, max_components=5000)
