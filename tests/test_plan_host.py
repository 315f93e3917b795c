"""The plan step on the host (idg_plan, include/idg_mi355x.h):
uvw tracks -> subgrid metadata.  CPU only.

* bit for bit a plain Python / numpy-float32 restatement of the algorithm
  (twin() below), on arcs of ellipses with bad rows, for every variant of
  w layers, A-term slots and subgrid length;
* an independent float64 check of the geometry: every row in exactly one
  subgrid or dropped, every channel of every row kernel_size / 2 cells inside
  its subgrid, every subgrid inside the grid;
* capacity, count-only and invalid-argument behaviour, thread independence;
* the conventions end to end through the CPU oracle: plan -> gridder ->
  subgrid FFT -> adder puts S^2 x the histogram of visibility cells on the
  grid.
"""
import ctypes

import numpy as np
import pytest

import idg_amd
import plan_cases as pc
from idg_amd._lib import PlanParamsStruct, lib
from oracle import METADATA_DTYPE

F = np.float32
INV_2PI = F(1.0 / (2.0 * np.pi))
G, S, K, B, T, C = 512, 32, 8, 12, 300, 8


def twin(G, S, image_size, w_step, uvw, baselines, wn, K, Tmax=128, A=0, W=1):
    """The algorithm in numpy float32 scalars and Python integers.  Returns
    (metadata, dropped, why): why[i] names what closed subgrid i ("geometry",
    "tmax", "slot", "layer", "invalid" or "end")."""
    B, T = uvw.shape[:2]
    wn0, wn1 = F(wn[0]), F(wn[-1])
    cells = F(image_size) * INV_2PI
    s0, s1 = wn0 * cells, wn1 * cells
    use_w = F(w_step) != 0
    if use_w:
        ws = ((F(0.5) * (wn0 + wn1)) * INV_2PI) * (F(1.0) / F(w_step))
    half = G // 2

    def fits(b):
        wx, wy = b[1] - b[0] + 1, b[3] - b[2] + 1
        if wx > S - K or wy > S - K:
            return None
        x, y = b[0] - (S - wx) // 2, b[2] - (S - wy) // 2
        if x < 0 or x + S > G or y < 0 or y + S > G:
            return None
        return x, y

    def step(u, v, w):
        if not (np.isfinite(u) and np.isfinite(v) and np.isfinite(w)):
            return None
        c = []
        for p in (u * s0, u * s1, v * s0, v * s1):
            assert p.dtype == F
            p = np.floor(p)
            if not abs(p) < F(2.0 ** 30):
                return None
            c.append(int(p) + half)
        b = (min(c[0], c[1]), max(c[0], c[1]), min(c[2], c[3]),
             max(c[2], c[3]))
        if fits(b) is None:
            return None
        layer = 0
        if use_w:
            lf = np.floor(w * ws)
            assert lf.dtype == F
            lf = F(0) if not lf > 0 else lf
            lf = F(W - 1) if lf > F(W - 1) else lf
            layer = int(lf)
        return b, layer

    md, why, dropped = [], [], 0
    with np.errstate(all="ignore"):
        for bl in range(B):
            cur = None   # [t0, n, slot, layer, box]

            def close(reason):
                nonlocal cur
                if cur is not None:
                    x, y = fits(cur[4])
                    md.append((0, bl * T + cur[0], cur[1], cur[2],
                               baselines[bl][0], baselines[bl][1], x, y,
                               cur[3]))
                    why.append(reason)
                    cur = None

            for t in range(T):
                s = step(*uvw[bl, t])
                if s is None:
                    close("invalid")
                    dropped += 1
                    continue
                box, layer = s
                slot = t // A if A else 0
                if cur is not None:
                    m = (min(cur[4][0], box[0]), max(cur[4][1], box[1]),
                         min(cur[4][2], box[2]), max(cur[4][3], box[3]))
                    reason = ("tmax" if cur[1] >= Tmax else
                              "slot" if slot != cur[2] else
                              "layer" if layer != cur[3] else
                              "geometry" if fits(m) is None else None)
                    if reason is None:
                        cur[1] += 1
                        cur[4] = m
                        continue
                    close(reason)
                cur = [t, 1, slot, layer, box]
            close("end")
    return np.array(md, dtype=METADATA_DTYPE).reshape(-1), dropped, why


@pytest.fixture(scope="module")
def tracks():
    return pc.arc_tracks(B, T, G, C)


def _plan(tracks, variant, **kw):
    uvw, bl, wn = tracks
    w_step, W, A, tmax = variant
    return idg_amd.plan(G, S, pc.IMAGE_SIZE, w_step, uvw, bl, wn, K, tmax, A,
                        W, **kw)


@pytest.fixture(scope="module")
def twins(tracks):
    uvw, bl, wn = tracks
    return {v: twin(G, S, pc.IMAGE_SIZE, v[0], uvw, bl, wn, K, v[3], v[2],
                    v[1]) for v in pc.VARIANTS}


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_plan_equals_the_twin(tracks, twins, variant):
    md, dropped = _plan(tracks, variant)
    ref, ref_dropped, why = twins[variant]
    assert md.dtype == idg_amd.METADATA_DTYPE
    assert md.size == ref.size
    assert np.array_equal(md.view(np.int32), ref.view(np.int32))
    assert dropped == ref_dropped == 4      # the NaN row, three at u = 1e7
    per_baseline = np.bincount(md["time_offset"] // T, minlength=B)
    assert per_baseline.min() >= 2
    lengths = md["nr_timesteps"]
    assert lengths.min() >= 1 and lengths.max() <= variant[3]


def test_every_closing_rule_is_exercised(twins):
    """What the twin says closed each subgrid: geometry and the 128-timestep
    cap without w layers or slots, a slot change with A-term slots, a layer
    change with w layers; lengths run from 1 to 128."""
    v0, vw, va, vwa, v1 = pc.VARIANTS
    assert {"geometry", "tmax", "invalid", "end"} <= set(twins[v0][2])
    assert "layer" in twins[vw][2] and "layer" in twins[vwa][2]
    assert "slot" in twins[va][2] and "slot" in twins[vwa][2]
    assert set(twins[v1][2]) <= {"tmax", "invalid", "end"}
    n = np.concatenate([twins[v][0]["nr_timesteps"] for v in (v0, vw, va,
                                                              vwa)])
    assert n.min() == 1 and n.max() == twins[v0][0]["nr_timesteps"].max() \
        == 128
    # more rules, more subgrids
    sizes = [twins[v][0].size for v in (v0, vw, va, vwa)]
    assert sizes[0] < sizes[1] < sizes[3] and sizes[0] < sizes[2] < sizes[3]
    assert twins[v1][0].size == B * T - 4


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_geometry_in_float64(tracks, variant):
    uvw, bl, wn = tracks
    md, dropped = _plan(tracks, variant)
    rows = uvw.reshape(-1, 3).astype(np.float64)
    covered = np.zeros(B * T, np.int64)
    margin = np.inf
    for m in md:
        r0, n = int(m["time_offset"]), int(m["nr_timesteps"])
        assert m["baseline_offset"] == 0 and n >= 1
        assert r0 // T == (r0 + n - 1) // T          # one baseline
        assert tuple(bl[r0 // T]) == (m["station1"], m["station2"])
        covered[r0:r0 + n] += 1
        x, y = int(m["x"]), int(m["y"])
        assert 0 <= x and x + S <= G and 0 <= y and y + S <= G
        assert 0 <= m["z"] < variant[1]
        if variant[2]:
            assert m["aterm_index"] == (r0 % T) // variant[2] == \
                ((r0 + n - 1) % T) // variant[2]
        k = wn.astype(np.float64)[None, :]
        U = rows[r0:r0 + n, 0:1] * k / (2 * np.pi) * pc.IMAGE_SIZE + G / 2
        V = rows[r0:r0 + n, 1:2] * k / (2 * np.pi) * pc.IMAGE_SIZE + G / 2
        margin = min(margin, (U - x).min(), (x + S - U).min(), (V - y).min(),
                     (y + S - V).min())
    assert covered.max() == 1
    assert int((covered == 0).sum()) == dropped == 4
    bad = np.flatnonzero(covered == 0)
    assert not np.isfinite(rows[bad[0], 1]) and np.all(rows[bad[1:], 0] == 1e7)
    # 0.01: float32 rounding of a product below 2,048 cells
    assert margin >= K / 2 - 0.01, margin
    # order: baseline-major, t0 ascending
    assert np.all(np.diff(md["time_offset"]) > 0)
    idg_amd.validate_metadata(md.size, S, C, 64, B * T,
                              int(md["aterm_index"].max()) + 1, md)


# ---- the C entry: capacity, counting, arguments, threads ------------------
def _params(**kw):
    p = PlanParamsStruct()
    p.struct_size = ctypes.sizeof(PlanParamsStruct)
    p.grid_size, p.subgrid_size, p.image_size = G, S, pc.IMAGE_SIZE
    p.w_step_in_lambda, p.nr_w_layers, p.kernel_size = 0.0, 1, K
    p.max_nr_timesteps_per_subgrid, p.nr_timesteps_per_aterm = 128, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _call(tracks, params, md=None, capacity=0, nthreads=1, nb=B, nt=T, nc=C):
    uvw, bl, wn = tracks
    counts = np.full(2, -7, np.int32)
    rc = lib.idg_plan(ctypes.cast(ctypes.pointer(params), ctypes.c_void_p),
                      nb, nt, bl.ctypes.data_as(ctypes.c_void_p),
                      uvw.ctypes.data_as(ctypes.c_void_p), nc,
                      wn.ctypes.data_as(ctypes.c_void_p),
                      None if md is None else md.ctypes.data_as(
                          ctypes.c_void_p), capacity,
                      counts.ctypes.data_as(ctypes.c_void_p), nthreads)
    return rc, counts


def test_capacity_below_the_need(tracks):
    full, dropped = _plan(tracks, pc.VARIANTS[0])
    rc, counts = _call(tracks, _params())           # NULL / 0: counts only
    assert rc == 0 and tuple(counts) == (full.size, dropped)
    cap = full.size // 2
    md = np.full((full.size + 3) * 9, 0x5a5a5a5a, np.int32)
    rc, counts = _call(tracks, _params(), md, cap)
    assert rc == 0 and tuple(counts) == (full.size, dropped)
    assert np.array_equal(md[:cap * 9], full.view(np.int32)[:cap * 9])
    assert np.all(md[cap * 9:] == 0x5a5a5a5a)
    # room to spare: nothing past the need is written
    md[:] = 0x5a5a5a5a
    rc, counts = _call(tracks, _params(), md, full.size + 3)
    assert rc == 0 and np.all(md[full.size * 9:] == 0x5a5a5a5a)
    assert np.array_equal(md[:full.size * 9], full.view(np.int32))


@pytest.mark.parametrize("variant", [pc.VARIANTS[0], pc.VARIANTS[3]])
def test_threads_give_identical_bytes(tracks, variant):
    a, da = _plan(tracks, variant, nthreads=1)
    b, db = _plan(tracks, variant, nthreads=5)
    c, dc = _plan(tracks, variant, nthreads=64)     # more threads than B
    assert a.tobytes() == b.tobytes() == c.tobytes() and da == db == dc


@pytest.mark.parametrize("bad", [
    dict(kernel_size=S), dict(kernel_size=-1), dict(subgrid_size=G + 2),
    dict(subgrid_size=0), dict(max_nr_timesteps_per_subgrid=0),
    dict(nr_w_layers=0), dict(nr_w_layers=(1 << 24) + 1),
    dict(nr_timesteps_per_aterm=-1),
    dict(struct_size=0), dict(struct_size=6), dict(struct_size=8),
])
def test_invalid_parameters(tracks, bad):
    rc, counts = _call(tracks, _params(**bad))
    assert rc == -1, bad                            # IDG_E_INVALID_ARGUMENT
    assert lib.idg_last_error()
    assert tuple(counts) == (-7, -7)


def test_invalid_sizes(tracks):
    for kw in (dict(nb=0), dict(nt=0), dict(nc=0), dict(nb=-1),
               dict(capacity=-1), dict(nb=1 << 16, nt=1 << 15),
               dict(capacity=4)):                   # NULL metadata, capacity 4
        rc, _ = _call(tracks, _params(), **kw)
        assert rc == -1, kw
    with pytest.raises(ValueError):                 # uvw rows of 2 floats
        idg_amd.plan(G, S, pc.IMAGE_SIZE, 0.0, tracks[0][:, :, :2],
                     tracks[1], tracks[2], K)


def test_larger_struct_with_zero_tail(tracks):
    class Newer(ctypes.Structure):
        _fields_ = [("known", PlanParamsStruct), ("extra", ctypes.c_uint32)]
    n = Newer()
    n.known = _params()
    n.known.struct_size = ctypes.sizeof(Newer)
    full, _ = _plan(tracks, pc.VARIANTS[0])
    counts = np.zeros(2, np.int32)
    uvw, bl, wn = tracks
    args = lambda: (B, T, bl.ctypes.data_as(ctypes.c_void_p),   # noqa: E731
                    uvw.ctypes.data_as(ctypes.c_void_p), C,
                    wn.ctypes.data_as(ctypes.c_void_p), None, 0,
                    counts.ctypes.data_as(ctypes.c_void_p), 1)
    assert lib.idg_plan(ctypes.cast(ctypes.pointer(n), ctypes.c_void_p),
                        *args()) == 0
    assert counts[0] == full.size
    n.extra = 1
    assert lib.idg_plan(ctypes.cast(ctypes.pointer(n), ctypes.c_void_p),
                        *args()) == -1


def test_a_baseline_without_subgrids_and_extreme_values():
    """Baseline 0 all invalid (NaN, inf, values whose products overflow the
    cell range or float32): md[0] belongs to baseline 1, whose time_offset is
    its row; nothing is undefined on the way."""
    uvw, bl, wn = pc.arc_tracks(3, 40, G, C, seed=3, bad_rows=False)
    uvw[0, :, 0] = np.resize(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38,
                                       1e12, -1e12, 2.0e11], F), 40)
    md, dropped = idg_amd.plan(G, S, pc.IMAGE_SIZE, 8.0, uvw, bl, wn, K,
                               nr_w_layers=4)
    ref, ref_dropped, _ = twin(G, S, pc.IMAGE_SIZE, 8.0, uvw, bl, wn, K, W=4)
    assert dropped == ref_dropped == 40
    assert np.array_equal(md.view(np.int32), ref.view(np.int32))
    assert md["time_offset"][0] == 40 and md["station1"][0] == bl[1][0]


def test_negative_w_lands_in_layer_0():
    uvw, bl, wn = pc.arc_tracks(2, 50, G, C, seed=4, bad_rows=False)
    uvw[0, :, 2] = -np.abs(uvw[0, :, 2]) - 1.0
    uvw[1, :, 2] = 1e4                              # far past the top layer
    md, _ = idg_amd.plan(G, S, pc.IMAGE_SIZE, 8.0, uvw, bl, wn, K,
                         nr_w_layers=4)
    assert np.all(md["z"][md["time_offset"] < 50] == 0)
    assert np.all(md["z"][md["time_offset"] >= 50] == 3)


# ---- conventions end to end through the CPU oracle ------------------------
def test_conventions_end_to_end_through_the_oracle(oracle_lib):
    """Measured here with the oracle on these inputs: 8.8e-7 of the grid's
    maximum (up to 36 visibilities on a cell); the bar is 4 x that."""
    o = pc.ONCELL
    case = pc.oncell_case()
    md, dropped = idg_amd.plan(o["G"], o["S"], o["image_size"], 0.0,
                               case["uvw"], case["baselines"], case["wn"],
                               o["K"], o["Tmax"])
    assert dropped == 0 and md.size >= 2 * o["B"]
    assert md["nr_timesteps"].sum() == o["B"] * o["T"]
    grid = pc.oncell_grid_through_the_oracle(oracle_lib, case, md)
    want = o["S"] ** 2 * case["hist"].astype(np.float64)
    assert case["hist"].max() > 20
    for pol in (0, 3):
        err = np.abs(grid[0, pol] - want).max() / want.max()
        print(f"pol {pol}: {err:.3e} of the maximum")
        assert err < 4 * 8.8e-7
    assert np.abs(grid[0, 1]).max() == 0.0 and np.abs(grid[0, 2]).max() == 0.0
    assert case["hist"].ravel()[np.argmax(np.abs(grid[0, 0]))] == \
        case["hist"].max()
