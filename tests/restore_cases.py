"""The restore step's contract (include/idg_mi355x.h) restated
in numpy, and the seeded cases of test_restore_host.py (host entry against
this restatement) and test_gpu_restore.py (device entry against the host
entry).  The restore is float32 with every operation rounded once; the beam
fit's normal equations are float64."""
import math

import numpy as np

from clean_cases import GUARD, fmaf

F = np.float32
REACH = 32           # the fit's window and the largest radius


# ---- the contract: restore -------------------------------------------------------
def restate(model, residual, taps, restored):
    """restored[y][x] = (residual ? residual[y][x] : 0) + acc, acc = the
    non-zero model pixels within +-R in row-major order, one fmaf each onto
    +0.  Walking the sources in row-major order and adding each one's
    footprint is that order at every output pixel."""
    G, R = model.shape[0], taps.shape[0] // 2
    acc = np.zeros((G, G), F)
    taken = ~(model == 0)                       # +-0 skipped, NaN taken
    for ys, xs in zip(*np.nonzero(taken)):      # (row-major)
        y0, y1 = max(ys - R, 0), min(ys + R, G - 1) + 1
        x0, x1 = max(xs - R, 0), min(xs + R, G - 1) + 1
        cut = acc[y0:y1, x0:x1]
        t = taps[y0 - ys + R:y1 - ys + R, x0 - xs + R:x1 - xs + R]
        with np.errstate(invalid="ignore", over="ignore"):
            cut[...] = fmaf(np.full(cut.shape, model[ys, xs], F), t, cut)
    with np.errstate(invalid="ignore", over="ignore"):
        restored[...] = (F(0) if residual is None else residual) + acc


# ---- the contract: beam ----------------------------------------------------------
def axes_to_abc(major, minor, pa):
    """a, b, c of exp(-(a dx^2 + 2 b dx dy + c dy^2)) with FWHMs major >=
    minor along / across the direction pa (from +x towards +y)."""
    lmaj = 4 * math.log(2) / major ** 2
    lmin = 4 * math.log(2) / minor ** 2
    cs, sn = math.cos(pa), math.sin(pa)
    return (lmaj * cs * cs + lmin * sn * sn, (lmaj - lmin) * sn * cs,
            lmaj * sn * sn + lmin * cs * cs)


def taps_of(abc, R):
    """The tap table in float64 (the caller rounds it)."""
    a, b, c = abc
    d = np.arange(-R, R + 1, dtype=np.float64)
    dy, dx = d[:, None], d[None, :]
    return np.exp(-(a * (dx * dx) + (2 * b) * (dx * dy) + c * (dy * dy)))


def gaussian_psf(Gp, abc):
    """A float32 Gaussian plane, centre (Gp // 2, Gp // 2) of value 1."""
    a, b, c = abc
    d = np.arange(Gp, dtype=np.float64) - Gp // 2
    dy, dx = d[:, None], d[None, :]
    return np.exp(-(a * dx * dx + 2 * b * dx * dy + c * dy * dy)).astype(F)


def fit_region(psf, level):
    """(dy, dx) of the pixels with q >= level that are 4-connected to the
    centre through such pixels, inside the psf and the +-32 window; in
    row-major order."""
    Gp = psf.shape[0]
    c = Gp // 2
    p0 = float(psf[c, c])
    seen = {(0, 0)}
    todo = [(0, 0)]
    while todo:
        dy, dx = todo.pop()
        for ny, nx in ((dy - 1, dx), (dy + 1, dx), (dy, dx - 1), (dy, dx + 1)):
            if (ny, nx) in seen or max(abs(ny), abs(nx)) > REACH:
                continue
            if not (0 <= c + ny < Gp and 0 <= c + nx < Gp):
                continue
            if float(psf[c + ny, c + nx]) / p0 >= level:
                seen.add((ny, nx))
                todo.append((ny, nx))
    return sorted(seen)


def fit_restated(psf, level=0.5):
    """a, b, c of the fit: the 3 x 3 normal equations of min sum w (a dx^2 +
    b2 dx dy + c dy^2 + ln q)^2, w = q^2, b2 = 2 b, accumulated in float64
    over the region in row-major order and solved by elimination."""
    c = psf.shape[0] // 2
    p0 = float(psf[c, c])
    m = [[0.0] * 4 for _ in range(3)]
    for dy, dx in fit_region(psf, level):
        if (dy, dx) == (0, 0):
            continue
        q = float(psf[c + dy, c + dx]) / p0
        w, ln = q * q, math.log(q)
        v = (float(dx * dx), float(dx * dy), float(dy * dy))
        for i in range(3):
            for j in range(3):
                m[i][j] += w * v[i] * v[j]
            m[i][3] -= w * ln * v[i]
    for k in range(3):
        pivot = max(range(k, 3), key=lambda i: abs(m[i][k]))
        m[k], m[pivot] = m[pivot], m[k]
        for i in range(k + 1, 3):
            f = m[i][k] / m[k][k]
            for j in range(k, 4):
                m[i][j] -= f * m[k][j]
    x = [0.0] * 3
    for k in (2, 1, 0):
        s = m[k][3] - sum(m[k][j] * x[j] for j in range(k + 1, 3))
        x[k] = s / m[k][k]
    return x[0], 0.5 * x[1], x[2]


# ---- seeded inputs ---------------------------------------------------------------
def case_taps(R, seed=0):
    """Positive float32 taps of a beam about as wide as R allows, centre 1."""
    if R == 0:
        return np.ones((1, 1), F)
    return taps_of(axes_to_abc(0.9 * R, 0.6 * R, 0.5 + seed), R).astype(F)


def case(G, R, model, residual=True, alias=False, seed=3):
    rng = np.random.default_rng(seed)
    res = rng.normal(size=(G, G)).astype(F) if residual else None
    return dict(G=G, R=R, model=np.ascontiguousarray(model, F), residual=res,
                taps=case_taps(R), alias=alias)


def _points(G, *pixels):
    m = np.zeros((G, G), F)
    for y, x, v in pixels:
        m[y, x] = v
    return m


def _random(G, fraction, seed):
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(G, G)).astype(F)      # both signs
    m[rng.uniform(size=(G, G)) >= fraction] = 0
    return m


def _dense(G, seed):
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.5, 1.5, (G, G)) * rng.choice([-1.0, 1.0], (G, G))
    return m.astype(F)


def _specials(G):
    """-0.0 (skipped), a NaN and an Inf (taken) and a few ordinary pixels; no
    second infinity, so nothing below makes a NaN of its own (whose sign bit
    would be the platform's, not the contract's)."""
    m = _points(G, (5, 5, 2.0), (6, 30, -1.5), (20, 20, np.nan),
                (30, 8, np.inf), (31, 9, 3.0), (12, 33, 1.0))
    m[12, 34] = F(-0.0)
    m[0, 0] = F(-0.0)
    return m


CASES = {
    "G8_R2_corners_and_middle": lambda: case(
        8, 2, _points(8, (0, 0, 1.0), (0, 7, -2.0), (7, 0, 3.0), (7, 7, 4.0),
                      (4, 3, 5.0))),
    "G37_R3_scalar_path": lambda: case(37, 3, _random(37, 0.02, 11)),
    "G40_R0": lambda: case(40, 0, _random(40, 0.05, 12)),
    "G48_R32_window_wider_than_image": lambda: case(
        48, 32, _random(48, 0.02, 13)),
    "G64_R5_dense": lambda: case(64, 5, _dense(64, 14)),
    "all_zero_model": lambda: case(40, 3, np.zeros((40, 40), F)),
    "minus_zero_nan_inf": lambda: case(40, 3, _specials(40)),
    "no_residual": lambda: case(37, 3, _random(37, 0.02, 15), residual=False),
    "restored_is_residual": lambda: case(40, 3, _random(40, 0.03, 16),
                                         alias=True),
}


# The device's tiles are 64 columns x 32 rows: 3 x 6 whole tiles and a
# remainder either way, non-zero pixels on both sides of every seam, and a
# dense block that covers the whole haloed window of tile (1, 1) (72 x 40
# pixels at R = 4), so that every round of that tile's scan fills its list
# (1024 entries).  G = 200 takes the float4 scan, G = 203 the scalar one.
TILE_COLS, TILE_ROWS = 64, 32


def _seams(G):
    rng = np.random.default_rng(G)
    m = np.zeros((G, G), F)
    for s in range(TILE_COLS, G, TILE_COLS):
        ys = rng.integers(0, G, 12)
        m[ys, s - 1] = rng.normal(size=12)
        m[ys, s] = rng.normal(size=12)
    for s in range(TILE_ROWS, G, TILE_ROWS):
        xs = rng.integers(0, G, 12)
        m[s - 1, xs] = rng.normal(size=12)
        m[s, xs] = rng.normal(size=12)
    for y in range(TILE_ROWS, G, TILE_ROWS):       # the corners of four tiles
        for x in range(TILE_COLS, G, TILE_COLS):
            m[y - 1:y + 1, x - 1:x + 1] = rng.uniform(1, 2, (2, 2))
    m[26:74, 58:138] = rng.uniform(0.5, 1.5, (48, 80))
    return m


LARGE = {
    "G200_R4_tile_seams": lambda: case(200, 4, _seams(200)),
    "G203_R4_tile_seams_scalar": lambda: case(203, 4, _seams(203)),
}


# ---- guarded buffers and runs ------------------------------------------------------
def buffers(c):
    """model, residual (if any) and restored between two guard rows each;
    restored is the residual's array when the case aliases them."""
    G = c["G"]

    def guarded(inner):
        a = np.full((G + 2, G), GUARD, F)
        a[1:-1] = inner
        return a
    b = dict(model=guarded(c["model"]))
    if c["residual"] is not None:
        b["residual"] = guarded(c["residual"])
    b["restored"] = b["residual"] if c["alias"] else guarded(0)
    return b


def guards_intact(b):
    return all(np.all(a[[0, -1]] == GUARD) for a in b.values())


def run_restatement(c):
    b = buffers(c)
    res = b["residual"][1:-1] if "residual" in b else None
    restate(b["model"][1:-1], res, c["taps"], b["restored"][1:-1])
    return b


def run_host(idg, c):
    b = buffers(c)
    res = b["residual"][1:-1] if "residual" in b else None
    out = idg.restore(b["model"][1:-1], res, taps=c["taps"],
                      out=b["restored"][1:-1])
    assert out is not None and out.ctypes.data == b["restored"][1:-1].ctypes.data
    return b


def same_bytes(a, b):
    """Names of the buffers() entries whose bytes differ."""
    return [k for k in a if a[k].tobytes() != b[k].tobytes()]
