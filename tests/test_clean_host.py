"""The host entry of the Hogbom minor cycle (idg_clean) against
the numpy restatement of its contract in clean_cases.py: every output compared
as bytes, guard rows included.  No device needed."""
import ctypes

import numpy as np
import pytest

import clean_cases as cc

F = np.float32


@pytest.fixture(scope="module")
def idg():
    import idg_amd
    return idg_amd


_runs = {}


def _run(idg, name):
    """(case, host buffers, restatement's buffers), made once."""
    if name not in _runs:
        c = cc.CASES[name]()
        _runs[name] = (c, cc.run_host(idg, c), cc.run_restatement(c))
    return _runs[name]


def _inner(b):
    return (b["residual"][1:-1], b["model"][1:-1], b["components"][1:-1],
            b["state"][0])


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_host_entry_is_the_restatement(idg, name):
    c, got, want = _run(idg, name)
    st = got["state"][0]
    print(f"{name}: n_components {st['n_components']} reason {st['reason']} "
          f"level {st['level']!r} peak {st['peak']!r} at {st['peak_index']}")
    assert cc.same_bytes(got, want) == []
    assert cc.guards_intact(got)


def test_dtypes_are_the_abis(idg):
    assert idg.COMPONENT_DTYPE == cc.COMPONENT and idg.STATE_DTYPE == cc.STATE
    assert ctypes.sizeof(idg.CleanParamsStruct) == 32
    assert idg.abi_version() == 1


# ---- what each case is for ----------------------------------------------------
def test_full_size_psf_runs_all_iterations(idg):
    c, got, _ = _run(idg, "G40_Gp40")
    res, model, comps, st = _inner(got)
    assert st["n_components"] == 25 and st["reason"] == 0
    assert tuple(comps[0])[:2] == (11, 27)
    assert np.abs(res).max() == st["peak"] < np.abs(c["residual"]).max()
    assert st["peak_index"] == np.abs(res).argmax()
    assert model.sum() != 0


@pytest.mark.parametrize("name,first", [("peak_at_0_0", (0, 0)),
                                        ("peak_at_last", (39, 39))])
def test_clipped_patches(idg, name, first):
    c, got, _ = _run(idg, name)
    res, model, comps, st = _inner(got)
    assert tuple(comps[0])[:2] == first
    # the patch is clipped: pixels beyond Gp / 2 of the corner keep their bytes
    # through the first component (a later one sits elsewhere)
    b = cc.buffers(c)
    idg.clean(b["residual"][1:-1], c["psf"], b["model"][1:-1],
              nr_iterations=1, components=b["components"][1:-1],
              state=b["state"], **cc.params(c))
    changed = b["residual"][1:-1] != c["residual"]
    ys, xs = np.nonzero(changed)
    G, Gp = c["G"], c["Gp"]
    lo = [max(f - Gp // 2, 0) for f in first]
    hi = [min(f - Gp // 2 + Gp, G) for f in first]
    inside = (hi[0] - lo[0]) * (hi[1] - lo[1])
    assert inside < Gp * Gp
    # (a pixel may keep its value where c * psf is below half an ulp of it)
    assert 0.9 * inside <= changed.sum() <= inside
    assert lo[0] <= ys.min() and ys.max() < hi[0]
    assert lo[1] <= xs.min() and xs.max() < hi[1]


def test_ties_go_to_the_lower_index(idg):
    _, got, _ = _run(idg, "tie_lower_index_wins")
    comps = _inner(got)[2]
    assert tuple(comps[0])[:2] == (10, 30) and tuple(comps[1])[:2] == (25, 5)
    _, got, _ = _run(idg, "tie_plus_minus")
    comps = _inner(got)[2]
    assert tuple(comps[0])[:2] == (8, 8) and comps[0]["value"] < 0
    assert tuple(comps[1])[:2] == (20, 3) and comps[1]["value"] > 0


def test_negative_peak_gives_a_negative_component(idg):
    c, got, _ = _run(idg, "negative_peak")
    res, model, comps, st = _inner(got)
    assert tuple(comps[0]) == (12, 14, F(0.2) * c["residual"][12, 14])
    assert comps[0]["value"] < 0 and model[12, 14] < 0


def test_nan_is_never_chosen_nor_altered(idg):
    c, got, _ = _run(idg, "nan_pixel")
    res, model, comps, st = _inner(got)
    n = st["n_components"]
    assert n == 10
    assert not any((y, x) == (30, 30) for y, x, _ in comps[:n])
    assert np.isnan(res[30, 30]) and np.isnan(res).sum() == 1
    assert st["peak_index"] != 30 * 40 + 30 and np.isfinite(st["peak"])


def test_mask_limits_the_search_only(idg):
    c, got, _ = _run(idg, "mask_hides_the_maximum")
    res, model, comps, st = _inner(got)
    n = st["n_components"]
    assert np.abs(c["residual"]).argmax() == 11 * 40 + 27
    assert all(c["mask"][y, x] != 0 for y, x, _ in comps[:n])
    # the subtraction reaches masked pixels
    assert np.any((res != c["residual"]) & (c["mask"] == 0))
    assert c["mask"].ravel()[st["peak_index"]] != 0


def test_all_zero_mask_stops_with_nothing_written(idg):
    c, got, _ = _run(idg, "mask_all_zero")
    res, model, comps, st = _inner(got)
    assert (st["reason"], st["n_components"]) == (2, 0)
    assert (st["peak"], st["peak_index"]) == (0, -1)
    assert res.tobytes() == c["residual"].tobytes()
    assert not model.any() and not comps["value"].any()


def test_threshold_stops_part_way(idg):
    c, got, _ = _run(idg, "threshold_reached")
    res, model, comps, st = _inner(got)
    n = st["n_components"]
    assert st["reason"] == 1 and 0 < n < 25 and st["level"] == 1.0
    assert st["peak"] <= 1.0 < abs(comps[n - 1]["value"]) / F(0.5)
    # the residual is that after the last component: n iterations, no more
    b = cc.buffers(c)
    idg.clean(b["residual"][1:-1], c["psf"], b["model"][1:-1],
              nr_iterations=int(n), components=b["components"][1:-1],
              state=b["state"], **cc.params(c))
    assert b["state"][0]["reason"] == 0
    assert b["residual"].tobytes() == got["residual"].tobytes()


def test_cycle_fraction_level_is_taken_once(idg):
    c, got, _ = _run(idg, "cycle_fraction")
    res, model, comps, st = _inner(got)
    first = np.abs(c["residual"]).max()
    assert st["level"] == F(F(0.5) * first) and st["started"] == 1
    assert st["reason"] == 1 and st["n_components"] > 1
    assert st["peak"] <= st["level"]


def test_components_full(idg):
    _, got, _ = _run(idg, "components_full")
    st = _inner(got)[3]
    assert (st["reason"], st["n_components"]) == (3, 4)


def test_zero_iterations_only_refresh_the_peak(idg):
    c, got, _ = _run(idg, "zero_iterations")
    res, model, comps, st = _inner(got)
    assert res.tobytes() == c["residual"].tobytes() and not model.any()
    assert not comps["value"].any()
    assert tuple(st)[:3] == (0, 0, 0) and st["level"] == 0
    assert st["peak"] == np.abs(c["residual"]).max()
    assert st["peak_index"] == np.abs(c["residual"]).argmax()


def test_three_calls_of_five_are_one_of_fifteen(idg):
    _, three, _ = _run(idg, "three_calls_of_5")
    _, one, _ = _run(idg, "one_call_of_15")
    assert cc.same_bytes(three, one) == []
    assert _inner(one)[3]["n_components"] == 15


def test_model_accumulates_in_order(idg):
    c, got, _ = _run(idg, "model_accumulates")
    res, model, comps, st = _inner(got)
    at = [(y, x) for y, x, _ in comps[:st["n_components"]]]
    assert at.count((17, 9)) >= 2
    want = c["model"].copy()
    for y, x, v in comps[:st["n_components"]]:
        want[y, x] = F(want[y, x] + v)
    assert model.tobytes() == want.tobytes()


def test_all_zero_residual_stops_at_threshold_zero(idg):
    _, got, _ = _run(idg, "all_zero_residual")
    st = _inner(got)[3]
    assert (st["reason"], st["n_components"], st["peak"]) == (1, 0, 0)
    assert st["peak_index"] == 0


# ---- the restatement's fmaf ----------------------------------------------------
def test_fmaf_restatement_on_a_million_triples(idg):
    """residual - c * psf over 4 planes of 500 x 500, PSF as large as the
    image and the peak forced to the centre, so that one iteration subtracts
    at every pixel: the host entry's fmaf against clean_cases.fmaf."""
    rng = np.random.default_rng(21)
    G = 500
    differing = 0
    for call in range(4):
        psf = (rng.normal(size=(G, G)) *
               2.0 ** rng.integers(-12, 4, (G, G))).astype(F)
        res = (rng.normal(size=(G, G)) *
               2.0 ** rng.integers(-12, 12, (G, G))).astype(F)
        res[G // 2, G // 2] = F(2.0 ** 20 * rng.uniform(1, 2))
        gain = F(rng.uniform(0.05, 1.0))
        c = F(gain * res[G // 2, G // 2])
        want = cc.fmaf(np.full((G, G), -c, F), psf, res)
        twice = (np.float64(-c) * psf.astype(np.float64)
                 + res.astype(np.float64)).astype(F)
        differing += int((twice != want).sum())
        got, _, comps, st = idg.clean(res.copy(), psf, gain=float(gain),
                                      nr_iterations=1, max_components=1)
        assert tuple(comps[0]) == (G // 2, G // 2, c)
        assert got.tobytes() == want.tobytes()
    print(f"fmaf: 10^6 triples; the plain float64 sum rounded to float32 "
          f"differs from the fused result in {differing}")


# ---- invalid arguments leave every buffer as it was ---------------------------
def _call(idg, c, b, params=None, **null):
    """idg_clean on buffers() with a raw parameter struct."""
    p = idg.CleanParamsStruct(ctypes.sizeof(idg.CleanParamsStruct), c["G"],
                              c["Gp"], c["max_components"], 3, c["gain"],
                              c["threshold"], c["cycle_fraction"])
    raw = bytearray(bytes(p))
    if params is not None:
        raw = params(p, raw)
    blob = (ctypes.c_char * len(raw)).from_buffer(raw)
    ptr = {"residual": b["residual"][1:-1], "psf": c["psf"],
           "model": b["model"][1:-1], "components": b["components"][1:-1],
           "state": b["state"]}
    args = [None if k in null else v.ctypes.data_as(ctypes.c_void_p)
            for k, v in ptr.items()]
    from idg_amd._lib import lib
    return lib.idg_clean(ctypes.cast(blob, ctypes.c_void_p), args[0], args[1],
                         None, *args[2:])


def _with(**fields):
    def edit(p, raw):
        for k, v in fields.items():
            setattr(p, k, v)
        return bytearray(bytes(p))
    return edit


def _grown(p, raw):
    p.struct_size += 4
    return bytearray(bytes(p)) + b"\x01\x00\x00\x00"


INVALID = {
    "struct_size_0": _with(struct_size=0),
    "struct_size_odd": _with(struct_size=30),
    "byte_past_the_known_fields": _grown,
    "grid_size_0": _with(grid_size=0, psf_size=0),
    "grid_size_too_large": _with(grid_size=16385),
    "psf_size_0": _with(psf_size=0),
    "psf_larger_than_grid": _with(psf_size=41),
    "gain_nan": _with(gain=float("nan")),
    "gain_inf": _with(gain=float("inf")),
    "threshold_inf": _with(threshold=float("inf")),
    "threshold_negative": _with(threshold=-1.0),
    "cycle_fraction_nan": _with(cycle_fraction=float("nan")),
    "cycle_fraction_negative": _with(cycle_fraction=-0.5),
    "nr_iterations_negative": _with(nr_iterations=-1),
    "max_components_negative": _with(max_components=-1),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_parameters(idg, name):
    c = cc.CASES["G40_Gp40"]()
    b, before = cc.buffers(c), cc.buffers(c)
    assert _call(idg, c, b, INVALID[name]) == -1     # IDG_E_INVALID_ARGUMENT
    assert cc.same_bytes(b, before) == []


@pytest.mark.parametrize("null", ["residual", "psf", "model", "components",
                                  "state"])
def test_null_buffer(idg, null):
    c = cc.CASES["G40_Gp40"]()
    b, before = cc.buffers(c), cc.buffers(c)
    assert _call(idg, c, b, **{null: True}) == -1
    assert cc.same_bytes(b, before) == []


@pytest.mark.parametrize("n", [-1, 26])
def test_state_out_of_range(idg, n):
    c = cc.CASES["G40_Gp40"]()
    b, before = cc.buffers(c), cc.buffers(c)
    b["state"]["n_components"] = before["state"]["n_components"] = n
    assert _call(idg, c, b) == -1
    assert cc.same_bytes(b, before) == []
    with pytest.raises(idg.IdgError):
        idg.clean(b["residual"][1:-1], c["psf"], b["model"][1:-1],
                  state=b["state"], components=b["components"][1:-1],
                  **cc.params(c))


def test_a_larger_struct_of_zeros_is_accepted(idg):
    c = cc.CASES["G40_Gp40"]()
    b = cc.buffers(c)

    def grown(p, raw):
        p.struct_size += 4
        return bytearray(bytes(p)) + bytes(4)
    assert _call(idg, c, b, grown) == 0
    assert b["state"][0]["n_components"] == 3


# ---- the plain-array helpers -----------------------------------------------------
def test_stokes_i_and_model_image(idg):
    rng = np.random.default_rng(3)
    image = rng.normal(size=(4, 6, 6, 2)).astype(F)
    i = idg.stokes_i(image)
    assert i.dtype == F and i.shape == (6, 6)
    assert np.array_equal(i, F(0.5) * (image[0, :, :, 0] + image[3, :, :, 0]))
    m = idg.model_image(i)
    assert m.dtype == F and m.shape == (4, 6, 6, 2)
    assert np.array_equal(m[0, :, :, 0], i) and np.array_equal(m[3, :, :, 0], i)
    assert not m[1:3].any() and not m[..., 1].any()
    assert np.array_equal(idg.stokes_i(m), i)
