"""The host entries of multi-scale CLEAN (idg_ms_*, idg_convolve_separable;
DESIGN.md §17) against the numpy restatement of their contract in
multiscale_cases.py: every output compared as bytes, guard rows included (the
taps to 1 ulp); Ns = 1 against the Hogbom entry; and the property the feature
is for, on an extended source.  No device needed."""
import ctypes
import json
import os

import numpy as np
import pytest

import clean_cases as cc
import multiscale_cases as mc
from conftest import REPO

F = np.float32


@pytest.fixture(scope="module")
def idg():
    import idg_amd
    return idg_amd


def test_dtypes_are_the_abis(idg):
    assert idg.MS_COMPONENT_DTYPE == mc.COMPONENT
    assert idg.MS_STATE_DTYPE == mc.STATE
    assert ctypes.sizeof(idg.MsParamsStruct) == 36 + 3 * 32


# ---- taps ------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0, 1, 4, 8, 16, 32, 64, 85, 2.5])
def test_taps_within_one_ulp_of_the_float64_restatement(idg, scale):
    taps, = idg.ms_scale_taps([scale])
    want = mc.scale_taps64(scale)
    assert taps.dtype == F and taps.size == 2 * mc.scale_radius(scale) + 1
    near = want.astype(F)
    assert np.all(np.abs(taps.astype(np.float64) - want) <= np.spacing(near))
    if scale == 0:
        assert taps.tobytes() == np.ones(1, F).tobytes()
    else:
        assert np.array_equal(taps, taps[::-1]) and abs(taps.sum() - 1) < 1e-6


def test_scales_refused(idg):
    for bad in (-1.0, float("nan"), 86.0, float("inf")):
        with pytest.raises(idg.IdgError) as e:
            idg.ms_scale_taps([bad])
        assert e.value.code == -1
    from idg_amd._lib import lib
    buf = np.zeros(8, F)
    assert lib.idg_ms_scale_taps(4.0, 2, buf.ctypes.data_as(
        ctypes.c_void_p)) == -1 and not buf.any()
    assert lib.idg_ms_scale_taps(4.0, 3, None) == -1


# ---- convolution -------------------------------------------------------------------
def _conv(idg, image, taps, in_place=False):
    """(tmp, out) allocations with their guard rows, through the host entry."""
    G = image.shape[0]
    tmp = mc.guarded(np.zeros((G, G), F))
    out = mc.guarded(image if in_place else np.zeros((G, G), F))
    src = mc.inner(out, (G, G)) if in_place else image
    got = idg.convolve_separable(src, taps, out=mc.inner(out, (G, G)),
                                 tmp=mc.inner(tmp, (G, G)))
    assert got.ctypes.data == mc.inner(out, (G, G)).ctypes.data
    return tmp, out


@pytest.mark.parametrize("name", sorted(mc.CONV))
def test_convolution_is_the_restatement(idg, name):
    image, scale = mc.CONV[name]()
    taps, = idg.ms_scale_taps([scale])
    G = image.shape[0]
    want_tmp, want = mc.convolve(image, taps)
    before = image.copy()
    tmp, out = _conv(idg, image, taps)
    assert image.tobytes() == before.tobytes()
    assert mc.inner(tmp, (G, G)).tobytes() == want_tmp.tobytes()
    assert mc.inner(out, (G, G)).tobytes() == want.tobytes()
    assert mc.guards_ok(tmp) and mc.guards_ok(out)
    _, again = _conv(idg, image, taps, in_place=True)
    assert again.tobytes() == out.tobytes()


def test_nonfinite_pixels_spread_as_they_are(idg):
    image, scale = mc.CONV["G36_nan_and_inf"]()
    taps, = idg.ms_scale_taps([scale])
    out = idg.convolve_separable(image, taps)
    r, G = taps.size // 2, 36
    assert np.isnan(out[G // 3 - r:G // 3 + r + 1,
                        G // 2 - r:G // 2 + r + 1]).all()
    assert np.isinf(out[G - 2, 1]) and np.isfinite(out[0, 0])


def test_a_delta_gives_the_outer_product(idg):
    taps, = idg.ms_scale_taps([16])
    image = np.zeros((40, 40), F)
    image[20, 17] = 1
    out = idg.convolve_separable(image, taps)
    assert np.array_equal(out[11:30, 8:27], np.outer(taps, taps))
    assert np.count_nonzero(out) == 19 * 19


def test_convolution_refusals(idg):
    image, taps = np.ones((6, 6), F), np.ones(3, F)
    other = np.zeros((6, 6), F)
    for kw in (dict(tmp=image), dict(out=other, tmp=other)):
        with pytest.raises(idg.IdgError) as e:
            idg.convolve_separable(image, taps, **kw)
        assert e.value.code == -1
    with pytest.raises(idg.IdgError):
        idg.convolve_separable(np.ones((120, 120), F), np.ones(99, F))
    assert image.tobytes() == np.ones((6, 6), F).tobytes() and not other.any()


# ---- prepare -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.PREP))
def test_prepare_is_the_restatement(idg, name):
    c = mc.PREP[name]()
    residual, psf, taps = mc.prep_inputs(c, idg)
    Ns, G, Gp = len(taps), c["G"], c["Gp"]
    want_planes, want_cross = mc.prepare(residual, psf, taps)
    planes = mc.guarded(np.zeros((Ns, G, G), F))
    cross = mc.guarded(np.zeros((Ns * (Ns + 1) // 2, Gp, Gp), F))
    tmp = mc.guarded(np.zeros((G, G), F))
    idg.ms_prepare(residual, psf, taps, planes=mc.inner(planes, (Ns, G, G)),
                   cross_psf=mc.inner(cross, want_cross.shape),
                   tmp=mc.inner(tmp, (G, G)))
    got_planes = mc.inner(planes, (Ns, G, G))
    got_cross = mc.inner(cross, want_cross.shape)
    assert got_planes.tobytes() == want_planes.tobytes()
    assert got_cross.tobytes() == want_cross.tobytes()
    assert got_planes[0].tobytes() == residual.tobytes()
    assert got_cross[0].tobytes() == psf.tobytes()
    assert mc.guards_ok(planes) and mc.guards_ok(cross) and mc.guards_ok(tmp)


def test_prepare_refusals(idg):
    c = mc.PREP["G8_Gp5_scale_16_wider_than_the_psf"]()
    residual, psf, taps = mc.prep_inputs(c, idg)
    planes, cross = idg.ms_prepare(residual, psf, taps)
    before = planes.copy(), cross.copy()
    for bad in (dict(taps=taps[::-1]),                       # radius[0] != 0
                dict(taps=[taps[0]] * 9),                     # Ns = 9
                dict(tmp=planes[1])):                         # overlap
        with pytest.raises((idg.IdgError, ValueError)):
            idg.ms_prepare(residual, psf, bad.get("taps", taps),
                           planes=planes, cross_psf=cross, tmp=bad.get("tmp"))
    with pytest.raises(idg.IdgError):
        idg.ms_prepare(psf, residual, taps)                   # Gp > G
    assert planes.tobytes() == before[0].tobytes()
    assert cross.tobytes() == before[1].tobytes()


# ---- the minor cycle -----------------------------------------------------------------
_runs = {}


def _run(idg, name):
    """(case, inputs, host buffers, restatement's buffers), made once."""
    if name not in _runs:
        c = mc.MS[name]()
        i = mc.ms_inputs(c, idg)
        _runs[name] = (c, i, mc.run_host(idg, c, i), mc.run_restatement(c, i))
    return _runs[name]


def _inner(c, b):
    Ns, G = len(c["scales"]), c["G"]
    return (mc.inner(b["planes"], (Ns, G, G)), mc.inner(b["model"], (G, G)),
            b["components"][1:-1], b["state"][0])


@pytest.mark.parametrize("name", sorted(mc.MS))
def test_minor_cycle_is_the_restatement(idg, name):
    c, i, got, want = _run(idg, name)
    st = got["state"][0]
    print(f"{name}: n_components {st['n_components']} reason {st['reason']} "
          f"level {st['level']!r} peak {st['peak']!r} at {st['peak_index']} "
          f"scale {st['peak_scale']}; scales used "
          f"{sorted(set(got['components'][1:-1]['scale'][:st['n_components']]))}")
    assert mc.same_bytes(got, want) == []
    assert mc.ms_guards_ok(got)


def test_border_case_takes_the_corners(idg):
    c, i, got, _ = _run(idg, "G8_Gp5_border_and_corners")
    comps, st = _inner(c, got)[2:]
    at = {(int(y), int(x)) for y, x, _, _ in comps[:st["n_components"]]}
    assert {(0, 0), (7, 7)} <= at


def test_large_scales_are_used_and_clipped(idg):
    c, i, got, _ = _run(idg, "G64_Gp33_four_scales_clipped")
    planes, model, comps, st = _inner(c, got)
    n = st["n_components"]
    assert {2, 3} <= set(comps["scale"][:n])
    # a footprint clipped at the image's edge
    assert any(s > 0 and (y < i["taps"][s].size // 2 or
                          x + i["taps"][s].size // 2 >= 64)
               for y, x, s, _ in comps[:n])


def test_footprint_is_split_across_the_device_tiles(idg):
    c, i, got, _ = _run(idg, "G260_Gp65_footprint_across_tiles")
    planes, model, comps, st = _inner(c, got)
    at = [tuple(int(v) for v in tuple(r)[:3]) for r in comps[:6]]
    assert (8, 256, 2) in at and (8, 256, 1) in at and (135, 255, 1) in at
    r = i["taps"][2].size // 2
    assert r == 5 and model[8 - r, 256 - r] != 0 and model[8 + r, 259] != 0
    assert np.count_nonzero(model[:8, :256]) and np.count_nonzero(
        model[8:, 256:])


def test_ties(idg):
    c, i, got, _ = _run(idg, "tie_between_scales_lower_scale_wins")
    comps = _inner(c, got)[2]
    assert tuple(comps[0])[:3] == (25, 5, 0)
    assert tuple(comps[1])[:3] == (10, 30, 1)
    c, i, got, _ = _run(idg, "tie_within_a_scale_lower_index_wins")
    comps = _inner(c, got)[2]
    assert tuple(comps[0])[:3] == (8, 8, 1) and comps[0]["value"] < 0
    assert tuple(comps[1])[:3] == (20, 3, 1) and comps[1]["value"] > 0


def test_nan_is_never_chosen(idg):
    c, i, got, _ = _run(idg, "nan_on_one_scale_only")
    planes, model, comps, st = _inner(c, got)
    n = st["n_components"]
    assert n == 8 and np.isnan(planes[1, 30, 30])
    assert np.isnan(planes).sum() == 1 and np.isfinite(model).all()
    assert not any((y, x, s) == (30, 30, 1) for y, x, s, _ in comps[:n])
    assert np.isfinite(st["peak"])


def test_mask_limits_the_search_on_every_scale(idg):
    c, i, got, _ = _run(idg, "mask_hides_the_maximum")
    planes, model, comps, st = _inner(c, got)
    n = st["n_components"]
    assert n > 0 and all(c["mask"][y, x] != 0 for y, x, _, _ in comps[:n])
    assert np.any((planes[0] != i["planes"][0]) & (c["mask"] == 0))
    assert c["mask"].ravel()[st["peak_index"]] != 0


def test_every_stop_reason(idg):
    reasons = {"still_running": 0, "stop_below_level": 1,
               "stop_cycle_fraction": 1, "stop_no_peak_mask_all_zero": 2,
               "stop_components_full": 3}
    for name, reason in reasons.items():
        c, i, got, _ = _run(idg, name)
        st = _inner(c, got)[3]
        assert st["reason"] == reason, name
    st = _inner(*_run(idg, "stop_below_level")[::2])[3]
    assert 0 < st["n_components"] < 60 and st["peak"] <= st["level"] == 1.0
    st = _inner(*_run(idg, "stop_no_peak_mask_all_zero")[::2])[3]
    assert (st["peak"], st["peak_index"], st["peak_scale"]) == (0, -1, -1)
    st = _inner(*_run(idg, "stop_components_full")[::2])[3]
    assert st["n_components"] == 4


def test_zero_iterations_only_refresh_the_peak(idg):
    c, i, got, _ = _run(idg, "zero_iterations")
    planes, model, comps, st = _inner(c, got)
    assert planes.tobytes() == i["planes"].tobytes() and not model.any()
    assert tuple(st)[:3] == (0, 0, 0) and st["level"] == 0
    s, at = mc.peak(i["planes"], i["weight"], None)
    assert (st["peak_scale"], st["peak_index"]) == (s, at) and st["peak"] > 0


def test_chunks_are_one_call(idg):
    _, _, three, _ = _run(idg, "chunks_3_4_5")
    _, _, one, _ = _run(idg, "one_call_of_12")
    assert mc.same_bytes(three, one) == []
    assert one["state"][0]["n_components"] == 12


# ---- refusals leave every buffer as it was --------------------------------------------
def _call(idg, c, i, b, edit=None, **null):
    """idg_ms_clean on ms_buffers() with a raw parameter struct."""
    Ns = len(c["scales"])
    p = idg.MsParamsStruct()
    p.struct_size = ctypes.sizeof(idg.MsParamsStruct)
    p.grid_size, p.psf_size, p.nr_scales = c["G"], c["Gp"], Ns
    p.max_components, p.nr_iterations = c["max_components"], 3
    p.gain, p.threshold, p.cycle_fraction = (c["gain"], c["threshold"],
                                             c["cycle_fraction"])
    for s in range(Ns):
        p.radius[s] = i["taps"][s].size // 2
        p.weight[s], p.inv_peak[s] = i["weight"][s], i["inv_peak"][s]
    raw = bytearray(bytes(p))
    if edit is not None:
        raw = edit(p, raw)
    blob = (ctypes.c_char * len(raw)).from_buffer(raw)
    table = np.concatenate(i["taps"])
    ptr = {"planes": b["planes"][1:-1], "cross": i["cross"], "taps": table,
           "mask": None, "model": b["model"][1:-1],
           "components": b["components"][1:-1], "state": b["state"]}
    args = [None if k in null or v is None
            else v.ctypes.data_as(ctypes.c_void_p) for k, v in ptr.items()]
    from idg_amd._lib import lib
    return lib.idg_ms_clean(ctypes.cast(blob, ctypes.c_void_p), *args)


def _with(**fields):
    def edit(p, raw):
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return bytearray(bytes(p))
    return edit


def _grown(p, raw):
    p.struct_size += 4
    return bytearray(bytes(p)) + b"\x01\x00\x00\x00"


INVALID = {
    "struct_size_0": _with(struct_size=0),
    "struct_size_odd": _with(struct_size=130),
    "byte_past_the_known_fields": _grown,
    "grid_size_0": _with(grid_size=0, psf_size=0),
    "grid_size_too_large": _with(grid_size=16385),
    "psf_size_0": _with(psf_size=0),
    "psf_larger_than_grid": _with(psf_size=65),
    "gain_nan": _with(gain=float("nan")),
    "threshold_inf": _with(threshold=float("inf")),
    "threshold_negative": _with(threshold=-1.0),
    "cycle_fraction_nan": _with(cycle_fraction=float("nan")),
    "cycle_fraction_negative": _with(cycle_fraction=-0.5),
    "nr_iterations_negative": _with(nr_iterations=-1),
    "max_components_negative": _with(max_components=-1),
    "nr_scales_0": _with(nr_scales=0),
    "nr_scales_9": _with(nr_scales=9),
    "radius_49": _with(radius=(1, 49)),
    "radius_negative": _with(radius=(2, -1)),
    "radius_0_not_0": _with(radius=(0, 1)),
    "weight_nan": _with(weight=(1, float("nan"))),
    "weight_inf": _with(weight=(0, float("inf"))),
    "inv_peak_inf": _with(inv_peak=(2, float("inf"))),
    "inv_peak_nan": _with(inv_peak=(0, float("nan"))),
}


@pytest.fixture(scope="module")
def still(idg):
    c = mc.MS["still_running"]()
    return c, mc.ms_inputs(c, idg)


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_parameters(idg, still, name):
    c, i = still
    b, before = mc.ms_buffers(c, i), mc.ms_buffers(c, i)
    assert _call(idg, c, i, b, INVALID[name]) == -1
    assert mc.same_bytes(b, before) == []


@pytest.mark.parametrize("null", ["planes", "cross", "taps", "model",
                                  "components", "state"])
def test_null_buffer(idg, still, null):
    c, i = still
    b, before = mc.ms_buffers(c, i), mc.ms_buffers(c, i)
    assert _call(idg, c, i, b, **{null: True}) == -1
    assert mc.same_bytes(b, before) == []


@pytest.mark.parametrize("n", [-1, 6])
def test_state_out_of_range(idg, still, n):
    c, i = still
    b, before = mc.ms_buffers(c, i), mc.ms_buffers(c, i)
    b["state"]["n_components"] = before["state"]["n_components"] = n
    assert _call(idg, c, i, b) == -1
    assert mc.same_bytes(b, before) == []


def test_a_valid_raw_call_runs(idg, still):
    c, i = still
    b = mc.ms_buffers(c, i)
    assert _call(idg, c, i, b) == 0
    assert b["state"][0]["n_components"] == 3


# ---- Ns = 1 is Hogbom ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_one_scale_is_hogbom(idg, name):
    c = cc.CASES[name]()
    want = cc.run_host(idg, c)
    b = cc.buffers(c)
    M = max(c["max_components"], 1)
    comps, state = np.zeros(M, mc.COMPONENT), np.zeros(1, mc.STATE)
    planes = cross = None
    for n in c["chunks"]:
        out = idg.clean_multiscale(
            b["residual"][1:-1], c["psf"], scales=(0,), model=b["model"][1:-1],
            mask=c["mask"], nr_iterations=n, components=comps, state=state,
            planes=planes, cross_psf=cross, **cc.params(c))
        planes, cross = out[4:]
    assert out[0].ctypes.data == b["residual"][1:-1].ctypes.data
    assert b["residual"].tobytes() == want["residual"].tobytes()
    assert b["model"].tobytes() == want["model"].tobytes()
    old = want["components"][1:-1]
    for k in ("y", "x", "value"):
        assert comps[k].tobytes() == old[k].tobytes()
    n = int(state[0]["n_components"])
    assert not comps["scale"][:n].any()
    for k in cc.STATE.names:
        assert state[k].tobytes() == want["state"][k].tobytes(), k
    assert state[0]["peak_scale"] == (0 if state[0]["peak_index"] >= 0 else -1)


# ---- what the feature is for --------------------------------------------------------------
def test_extended_source_takes_fewer_than_half_the_components(idg):
    """The float64 sketch of the algorithm took 217 components with scales
    (0, 4, 8, 16) against 1,069 with (0,) on a field of this kind."""
    dirty, psf = mc.property_field()
    counts = {}
    for scales in ((0, 4, 8, 16), (0,)):
        res, model, comps, state, planes, cross = idg.clean_multiscale(
            dirty.copy(), psf, scales=scales, **mc.PROPERTY)
        st = state[0]
        counts[scales] = int(st["n_components"])
        print(f"scales {scales}: {st['n_components']} components, reason "
              f"{st['reason']}, level {st['level']!r}, max |planes[0]| "
              f"{np.abs(planes[0]).max()!r}, model sum {model.sum()!r}")
        assert st["reason"] == 1
        assert np.abs(planes[0]).max() <= st["level"]
        assert res.tobytes() == planes[0].tobytes()
    out = os.path.join(REPO, "profiles", "multiscale")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "parity.json"), "w") as f:
        json.dump({"field": "multiscale_cases.property_field",
                   "dirty_peak": float(np.abs(dirty).max()),
                   **mc.PROPERTY,
                   "components_scales_0_4_8_16": counts[(0, 4, 8, 16)],
                   "components_scales_0": counts[(0,)]}, f, indent=1)
        f.write("\n")
    assert 2 * counts[(0, 4, 8, 16)] < counts[(0,)]
