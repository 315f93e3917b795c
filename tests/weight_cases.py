"""The imaging-weight contract restated in numpy, and the
inputs of its tests (test_weight_host.py on the CPU, test_gpu_weight.py on
the GPU).  Every float step below is one float32 operation in the order the
contract states; the density is a sum of uint64."""
import math

import numpy as np

import plan_cases as pc

F = np.float32
INV_2PI = F(0.15915494309189535)
QLOG2 = -20
SCHEMES = ("natural", "uniform", "briggs")


# ---- the restatement -------------------------------------------------------
def rows_of(md, s):
    """Rows of subgrid s (include/idg_mi355x.h)."""
    r0 = (int(md["baseline_offset"][s]) - int(md["baseline_offset"][0])
          + int(md["time_offset"][s]))
    return r0, r0 + int(md["nr_timesteps"][s])


def cover(md, rows):
    """How many subgrids cover each row."""
    n = np.zeros(rows, np.int64)
    for s in range(md.size):
        a, b = rows_of(md, s)
        n[a:b] += 1
    return n


def cells(G, image_size, uvw, wn):
    """X, Y [rows, C] int64 and whether the cell is finite and in the grid."""
    uvw = uvw.reshape(-1, 3)
    scale = wn.astype(F) * (F(image_size) * INV_2PI)           # [C]
    out = []
    with np.errstate(all="ignore"):
        for k in (0, 1):
            p = (uvw[:, k, None] * scale[None, :]).astype(F)
            p = np.floor((p + F(0.5)).astype(F))
            ok = np.abs(p) < F(2.0 ** 30)
            out.append((np.where(ok, p, 0).astype(np.int64) + G // 2, ok))
    (X, okx), (Y, oky) = out
    ok = okx & oky & (X >= 0) & (X < G) & (Y >= 0) & (Y < G)
    return X, Y, ok


def quantise(w, qlog2=QLOG2):
    w = w.astype(F)
    with np.errstate(all="ignore"):
        scaled = np.ldexp(w, -qlog2).astype(F)
        live = np.isfinite(w) & (w > 0) & (scaled < F(2.0 ** 40))
        return np.where(live, np.rint(np.where(live, scaled, 0)), 0).astype(
            np.uint64)


def sample_q(G, image_size, uvw, wn, weights, qlog2=QLOG2):
    """q [rows, C] (0: flagged or off the grid), X, Y."""
    X, Y, ok = cells(G, image_size, uvw, wn)
    q = np.where(ok, quantise(weights.reshape(X.shape), qlog2), 0).astype(
        np.uint64)
    return q, X, Y


def density(G, image_size, uvw, wn, weights, md, qlog2=QLOG2, into=None):
    d = np.zeros((G, G), np.uint64) if into is None else into.copy()
    q, X, Y = sample_q(G, image_size, uvw, wn, weights, qlog2)
    q = q * cover(md, q.shape[0]).astype(np.uint64)[:, None]
    live = q > 0
    np.add.at(d, (Y[live], X[live]), q[live])
    return d


def counts(d, hermitian=True):
    n = d.copy()
    if hermitian:
        n[1:, 1:] += d[1:, 1:][::-1, ::-1]
    return n


def D_of(d, qlog2=QLOG2, hermitian=True):
    return np.ldexp(counts(d, hermitian).astype(F), qlog2).astype(F)


def briggs_scale(robust):
    r = 5.0 * math.pow(10.0, -float(F(robust)))
    return r * r


def scheme_ab(d, scheme, robust=0.0, qlog2=QLOG2, hermitian=True):
    """(a, b) as float32, the Briggs sums exact (math.fsum)."""
    if scheme == "natural":
        return F(1), F(0)
    if scheme == "uniform":
        return F(0), F(1)
    D = D_of(d, qlog2, hermitian).astype(np.float64).ravel()
    sd, sd2 = math.fsum(D), math.fsum(D * D)
    return F(1), F(briggs_scale(robust) * sd / sd2) if sd2 > 0 else F(0)


def apply(G, image_size, uvw, wn, weights, md, d, a, b, vis=None,
          qlog2=QLOG2, hermitian=True, iw=None, out=None):
    """(imaging_weights [rows, C], out [rows, C, 4, 2], sum f (exact, as a
    float), number of covered samples); iw / out: what the buffers held."""
    q, X, Y = sample_q(G, image_size, uvw, wn, weights, qlog2)
    rows, C = q.shape
    w = weights.reshape(rows, C).astype(F)
    D = D_of(d, qlog2, hermitian)[np.clip(Y, 0, G - 1), np.clip(X, 0, G - 1)]
    with np.errstate(all="ignore"):
        den = (F(a) + (F(b) * D).astype(F)).astype(F)
        f = np.where(q > 0, (w / den).astype(F), F(0)).astype(F)
    if vis is None:
        o = np.zeros((rows, C, 4, 2), F)
        o[:, :, 0, 0] = f
        o[:, :, 3, 0] = f
    else:
        with np.errstate(all="ignore"):
            o = (f[:, :, None, None] * vis.reshape(rows, C, 4, 2)).astype(F)
        o[q == 0] = 0
    n = cover(md, rows)
    cov = n > 0
    iw = np.zeros((rows, C), F) if iw is None else iw.reshape(rows, C).copy()
    out = (np.zeros((rows, C, 4, 2), F) if out is None
           else out.reshape(rows, C, 4, 2).copy())
    iw[cov] = f[cov]
    out[cov] = o[cov]
    total = math.fsum((f.astype(np.float64) * n[:, None]).ravel())
    return iw, out, total, int(n.sum()) * C


def inside_box(case):
    """(live samples inside their subgrid's S x S box, live samples)."""
    q, X, Y = sample_q(case["G"], case["image_size"], case["uvw"], case["wn"],
                       case["weights"])
    md, S, inside, live = case["md"], case["S"], 0, 0
    for s in range(md.size):
        a, b = rows_of(md, s)
        x0, y0 = int(md["x"][s]), int(md["y"][s])
        m = q[a:b] > 0
        i = ((X[a:b] >= x0) & (X[a:b] < x0 + S) & (Y[a:b] >= y0)
             & (Y[a:b] < y0 + S))
        inside += int((i & m).sum())
        live += int(m.sum())
    return inside, live


def ulps_apart(x, y):
    """Distance in float32 units in the last place (same sign, finite)."""
    return abs(int(np.array(x, F).view(np.int32))
               - int(np.array(y, F).view(np.int32)))


# ---- inputs ----------------------------------------------------------------
def weights_for(rows, C, seed=2):
    return np.random.default_rng(seed).uniform(0.25, 4.0, (rows, C)).astype(F)


def vis_for(rows, C, seed=3):
    return np.random.default_rng(seed).normal(size=(rows, C, 4, 2)).astype(F)


def planned(B=12, T=300, G=512, C=8, S=32, kernel_size=8, Tmax=128,
            w_step=0.0, W=1, seed=1):
    """arc_tracks under the host plan: a dict with uvw [B*T, 3], wn, md,
    weights, vis and the geometry."""
    import idg_amd
    uvw, base, wn = pc.arc_tracks(B, T, G, C=C, seed=seed)
    md, _ = idg_amd.plan(G, S, pc.IMAGE_SIZE, w_step, uvw, base, wn,
                         kernel_size, Tmax, 0, W)
    return dict(G=G, S=S, C=C, image_size=pc.IMAGE_SIZE,
                uvw=np.ascontiguousarray(uvw.reshape(-1, 3)), wn=wn, md=md,
                weights=weights_for(B * T, C), vis=vis_for(B * T, C))


def generated(stations=4, timeslots=2, T=16, C=5, G=512, S=32):
    """The generator's observation: its subgrid coordinates are drawn at
    random, unrelated to uvw, so every sample lies outside its subgrid's box."""
    import idg_amd
    g = idg_amd.generate(stations, timeslots, T, C, G, S,
                         want=("uvw", "wavenumbers", "metadata"))
    rows = g["uvw"].shape[0] * T
    return dict(G=G, S=S, C=C, image_size=idg_amd.IMAGE_SIZE,
                uvw=np.ascontiguousarray(g["uvw"].reshape(-1, 3)),
                wn=g["wavenumbers"], md=g["metadata"],
                weights=weights_for(rows, C), vis=vis_for(rows, C))


def oncell(weights=None):
    """plan_cases.oncell_case under the host plan, unit weights."""
    import idg_amd
    o, case = pc.ONCELL, pc.oncell_case()
    md, dropped = idg_amd.plan(o["G"], o["S"], o["image_size"], 0.0,
                               case["uvw"], case["baselines"], case["wn"],
                               o["K"], o["Tmax"])
    assert dropped == 0
    rows = o["B"] * o["T"]
    return dict(G=o["G"], S=o["S"], C=1, image_size=o["image_size"],
                uvw=np.ascontiguousarray(case["uvw"].reshape(-1, 3)),
                wn=case["wn"], md=md, hist=case["hist"], case=case,
                weights=(np.ones((rows, 1), F) if weights is None
                         else weights), vis=case["vis"])


def one_cell(nr_subgrids=8, T=40, C=16, G=256, S=32, cell=(140, 97)):
    """Every sample of every subgrid in one uv cell: u, v put channel 0 on the
    cell's centre and the band is too narrow to leave it."""
    wn = pc.wavenumbers(C, df=1.0e3)
    per_cell = 1.0 / (float(wn[0]) / (2 * np.pi) * pc.IMAGE_SIZE)
    rows = nr_subgrids * T
    uvw = np.zeros((rows, 3), F)
    uvw[:, 0] = (cell[0] - G // 2) * per_cell
    uvw[:, 1] = (cell[1] - G // 2) * per_cell
    md = np.zeros(nr_subgrids, dtype=pc_metadata_dtype())
    md["time_offset"] = np.arange(nr_subgrids) * T
    md["nr_timesteps"] = T
    md["station2"] = 1
    md["x"] = cell[0] - S // 2
    md["y"] = cell[1] - S // 2
    return dict(G=G, S=S, C=C, image_size=pc.IMAGE_SIZE, uvw=uvw, wn=wn,
                md=md, weights=weights_for(rows, C), vis=vis_for(rows, C),
                cell=cell)


def pc_metadata_dtype():
    import idg_amd
    return idg_amd.METADATA_DTYPE


FLAG_KINDS = ("zero", "negative", "nan", "too_large", "nan_vis_behind_zero",
              "off_grid")


def flagged(case):
    """A copy of `case` with one covered sample (or row) of each kind of
    FLAG_KINDS, and {kind: (row, channel)}; off_grid moves a row's u after
    the plan, so the metadata still covers it."""
    c = dict(case)
    w, vis, uvw = case["weights"].copy(), case["vis"].copy(), \
        case["uvw"].copy()
    rows = np.flatnonzero(cover(case["md"], w.shape[0]) > 0)
    # rows whose samples are all on the grid to begin with
    _, _, ok = cells(case["G"], case["image_size"], uvw, case["wn"])
    rows = rows[ok[rows].all(axis=1)]
    pick = rows[np.linspace(0, rows.size - 1, len(FLAG_KINDS) + 2)
                .astype(int)[1:-1]]
    C = w.shape[1]
    where = {k: (int(r), int(i % C)) for i, (k, r) in
             enumerate(zip(FLAG_KINDS, pick))}
    w[where["zero"]] = 0.0
    w[where["negative"]] = -1.5
    w[where["nan"]] = np.nan
    w[where["too_large"]] = 2.0 ** 20
    w[where["nan_vis_behind_zero"]] = 0.0
    vis[where["nan_vis_behind_zero"]] = np.nan
    uvw[where["off_grid"][0], 0] = 1e7
    c.update(weights=w, vis=vis, uvw=uvw)
    return c, where
