"""The host side of the restore step (idg_beam_fit, idg_beam_from_axes,
idg_beam_radius, idg_beam_taps, idg_restore) against the numpy
restatement of its contract in restore_cases.py: the restored plane compared
as bytes, guard rows included; the fit against the float64 restatement of its
normal equations.  No device needed."""
import ctypes
import json
import math
import os
import struct

import numpy as np
import pytest

import restore_cases as rc

F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def idg():
    import idg_amd
    return idg_amd


_runs = {}


def _run(idg, name):
    """(case, host buffers, restatement's buffers), made once."""
    if name not in _runs:
        c = rc.CASES[name]()
        _runs[name] = (c, rc.run_host(idg, c), rc.run_restatement(c))
    return _runs[name]


# ---- 1. the host entry is the restatement ---------------------------------------
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_host_entry_is_the_restatement(idg, name):
    c, got, want = _run(idg, name)
    print(f"{name}: {int((~(c['model'] == 0)).sum())} sources, restored "
          f"range [{np.nanmin(got['restored'][1:-1])!r}, "
          f"{np.nanmax(got['restored'][1:-1])!r}]")
    assert rc.same_bytes(got, want) == []
    assert rc.guards_intact(got)
    # the inputs keep their bytes (restored may be the residual)
    assert got["model"][1:-1].tobytes() == c["model"].tobytes()
    if c["residual"] is not None and not c["alias"]:
        assert got["residual"][1:-1].tobytes() == c["residual"].tobytes()


def test_structs_are_the_abis(idg):
    assert ctypes.sizeof(idg.BeamStruct) == 56
    assert ctypes.sizeof(idg.RestoreParamsStruct) == 12


def test_cases_do_what_they_are_for(idg):
    c, got, _ = _run(idg, "G8_R2_corners_and_middle")
    out = got["restored"][1:-1]
    # a lone component of flux f restores to residual + f at its pixel
    assert out[0, 0] == c["residual"][0, 0] + F(1.0)
    assert out[7, 7] == c["residual"][7, 7] + F(4.0)
    c, got, _ = _run(idg, "G40_R0")
    assert np.array_equal(got["restored"][1:-1], c["residual"] + c["model"])
    c, got, _ = _run(idg, "all_zero_model")
    assert np.array_equal(got["restored"][1:-1], c["residual"] + F(0))
    c, got, _ = _run(idg, "no_residual")
    assert np.count_nonzero(got["restored"][1:-1]) > np.count_nonzero(
        c["model"])
    c, got, _ = _run(idg, "G64_R5_dense")
    assert np.count_nonzero(c["model"]) == 64 * 64
    c, got, _ = _run(idg, "minus_zero_nan_inf")
    out = got["restored"][1:-1]
    # -0.0 alone adds nothing: far from the other sources the plane is the
    # residual; the NaN and the Inf spread over their footprints only
    assert out[0, 0] == c["residual"][0, 0] + F(0)
    assert np.isnan(out[17:24, 17:24]).all() and np.isnan(out).sum() == 49
    assert np.isinf(out[27:34, 5:12]).all() and np.isinf(out).sum() == 49


def test_minus_zero_residual_plus_zero_is_plus_zero(idg):
    """The final add is made even where nothing was accumulated: -0.0f + 0.0f
    is +0.0f."""
    model = np.zeros((8, 8), F)
    residual = np.full((8, 8), -0.0, F)
    out = idg.restore(model, residual, taps=rc.case_taps(2))
    assert not np.signbit(out).any()


# ---- 2. refusals -------------------------------------------------------------------
def _raw(idg, G, R, model, residual, taps, restored, struct_size=None):
    from idg_amd._lib import lib
    p = idg.RestoreParamsStruct()
    p.struct_size = (ctypes.sizeof(p) if struct_size is None else struct_size)
    p.grid_size, p.radius = G, R

    def ptr(a):
        if a is None or isinstance(a, int):
            return a
        return a.ctypes.data_as(ctypes.c_void_p)
    return lib.idg_restore(ctypes.byref(p), ptr(model), ptr(residual),
                           ptr(taps), ptr(restored))


def test_refusals_leave_the_buffers(idg):
    c = rc.CASES["G37_R3_scalar_path"]()
    G, R = c["G"], c["R"]
    b = rc.buffers(c)
    taps = c["taps"].copy()
    before = {k: v.copy() for k, v in b.items()}
    m, r, o = b["model"][1:-1], b["residual"][1:-1], b["restored"][1:-1]
    bad_taps = taps.copy()
    bad_taps[1, 2] = np.inf
    nan_taps = taps.copy()
    nan_taps[0, 0] = np.nan
    # a plane that starts inside another one
    inside_r = b["residual"].reshape(-1)[G + 5:]
    wide = np.zeros((G + 1) * G, F)
    refusals = {
        "null model": (G, R, None, r, taps, o),
        "null taps": (G, R, m, r, None, o),
        "null restored": (G, R, m, r, taps, None),
        "G = 0": (0, R, m, r, taps, o),
        "G = 16385": (16385, R, m, r, taps, o),
        "R = -1": (G, -1, m, r, taps, o),
        "R = 33": (G, 33, m, r, taps, o),
        "restored is the model": (G, R, m, r, taps, m),
        "residual is the model": (G, R, m, m, taps, o),
        "restored overlaps the residual in part": (G, R, m, r, taps, inside_r),
        "restored overlaps the model in part": (
            G, R, m, r, taps, b["model"].reshape(-1)[5:]),
        "taps inside restored": (G, R, m, r, wide[3:], wide),
        "taps inside the model": (G, R, wide, r, wide[G:], o),
        "a tap is infinite": (G, R, m, r, bad_taps, o),
        "a tap is a NaN": (G, R, m, r, nan_taps, o),
    }
    for what, args in refusals.items():
        assert _raw(idg, *args) == -1, what
        for k in b:
            assert b[k].tobytes() == before[k].tobytes(), what
        assert not wide.any(), what
    for size in (0, 2, 6, 1 << 17):
        assert _raw(idg, G, R, m, r, taps, o, struct_size=size) == -1
    # through the Python entry: the message says which
    with pytest.raises(idg.IdgError, match="overlap") as e:
        idg.restore(m, r, taps=taps, out=m)
    assert e.value.code == -1
    with pytest.raises(idg.IdgError, match="not finite"):
        idg.restore(m, r, taps=bad_taps, out=o)
    with pytest.raises(ValueError):
        idg.restore(m, r, out=o)
    with pytest.raises(ValueError):
        idg.restore(m, r, taps=taps, beam=idg.beam_from_axes(3, 2, 0.5))
    for k in b:
        assert b[k].tobytes() == before[k].tobytes()
    # and the call they all refuse runs as it stands
    assert _raw(idg, G, R, m, r, taps, o) == 0
    assert _raw(idg, G, R, m, r, taps, r) == 0


# ---- 3. the fit -----------------------------------------------------------------------
AXES = [(3.0, 2.0, 0.5), (8.0, 3.0, -1.2), (4.0, 4.0, 0.0)]
# The float64 restatement's own error against the true a, b, c on a float32
# Gaussian of 65 x 65 pixels, max over the three of |difference| / the
# largest of |a|, |b|, |c|: measured here on the CPU (5.84e-8, 1.37e-8,
# 5.77e-9; the float32 rounding of the psf), written with a little room.  The
# library is held to ten times it; profiles/restore/fit.json has the same
# figures.
RESTATED_ERROR = {AXES[0]: 5.9e-8, AXES[1]: 1.4e-8, AXES[2]: 5.8e-9}


def _error(got, true):
    scale = max(abs(v) for v in true)
    return max(abs(g - t) for g, t in zip(got, true)) / scale


def _bits(beam):
    return struct.pack("<6d", *beam)


@pytest.mark.parametrize("axes", AXES)
def test_fit_of_a_gaussian(idg, axes):
    true = rc.axes_to_abc(*axes)
    psf = rc.gaussian_psf(65, true)
    want = rc.fit_restated(psf, 0.5)
    beam = idg.beam_fit(psf)
    got = (beam.a, beam.b, beam.c)
    figures = {"axes": axes, "region_pixels": len(rc.fit_region(psf, 0.5)),
               "restated_error": _error(want, true),
               "library_error": _error(got, true),
               "library_against_restated": _error(got, want)}
    print("beam fit: " + json.dumps(figures))
    # the same double arithmetic: 1e-10 relative, component by component (b
    # of the round beam is 0: there, relative to a)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-10 * (abs(w) if w != 0 else abs(want[0]))
    assert figures["restated_error"] <= RESTATED_ERROR[axes]
    assert figures["library_error"] <= 10 * RESTATED_ERROR[axes]
    # the derived fields describe the same form
    assert beam.major >= beam.minor > 0
    assert -math.pi / 2 < beam.pa <= math.pi / 2
    assert abs(beam.major - axes[0]) <= 1e-6 * axes[0]
    assert abs(beam.minor - axes[1]) <= 1e-6 * axes[1]
    if axes[0] != axes[1]:
        assert abs(beam.pa - axes[2]) <= 1e-6
    back = idg.beam_from_axes(beam.major, beam.minor, beam.pa)
    assert _error(back[:3], got) <= 1e-12


def test_fit_json_has_the_figures_of_this_file():
    with open(os.path.join(REPO, "profiles", "restore", "fit.json")) as f:
        rec = json.load(f)
    assert {tuple(r["axes"]): r["restated_error_bar"]
            for r in rec["cases"]} == RESTATED_ERROR


@pytest.mark.parametrize("axes", AXES)
def test_a_detached_lobe_changes_no_bit(idg, axes):
    psf = rc.gaussian_psf(65, rc.axes_to_abc(*axes))
    plain = idg.beam_fit(psf)
    lobed = psf.copy()
    lobed[32, 42] = 0.7           # above the level, ten pixels from the centre
    lobed[22, 32] = 0.7
    assert rc.fit_region(lobed, 0.5) == rc.fit_region(psf, 0.5)
    assert _bits(idg.beam_fit(lobed)) == _bits(plain)
    # (a lobe joined to the main one does change it)
    lobed[32, 33:43] = 0.7
    assert _bits(idg.beam_fit(lobed)) != _bits(plain)


def test_fit_takes_the_psf_as_it_is(idg):
    """Not normalised (q divides by the centre), even or odd Gp, Gp smaller
    than the window, another level."""
    true = rc.axes_to_abc(3.0, 2.0, 0.5)
    for Gp in (9, 12, 64, 200):
        psf = rc.gaussian_psf(Gp, true)
        want = rc.fit_restated(psf, 0.5)
        got = idg.beam_fit(psf)[:3]
        assert _error(got, want) <= 1e-10
    psf = rc.gaussian_psf(65, true)
    scaled = (psf * F(4.0)).astype(F)          # exact: a power of two
    assert _bits(idg.beam_fit(scaled)) == _bits(idg.beam_fit(psf))
    got = idg.beam_fit(psf, level=0.2)[:3]
    assert _error(got, rc.fit_restated(psf, 0.2)) <= 1e-10
    assert len(rc.fit_region(psf, 0.2)) > len(rc.fit_region(psf, 0.5))


def _raw_fit(idg, psf_size, psf, level, struct_size=56):
    from idg_amd._lib import lib
    b = idg.BeamStruct()
    b.struct_size = struct_size
    b.a, b.b, b.c, b.major, b.minor, b.pa = 1.5, 2.5, 3.5, 4.5, 5.5, 6.5
    before = bytes(b)
    rc_ = lib.idg_beam_fit(psf_size,
                           None if psf is None else
                           psf.ctypes.data_as(ctypes.c_void_p),
                           level, ctypes.byref(b))
    return rc_, bytes(b) == before


def test_fit_refusals(idg):
    from idg_amd._lib import lib
    good = rc.gaussian_psf(65, rc.axes_to_abc(3.0, 2.0, 0.5))
    delta = np.zeros((65, 65), F)
    delta[32, 32] = 1.0
    flat = np.ones((80, 80), F)
    line = delta.copy()
    line[32, 29:36] = 0.8                       # dy = 0 everywhere: singular
    ring = delta.copy()
    ring[31:34, 31:34] = 1.5                    # rises away from the centre
    ring[32, 32] = 1.0

    def centre(v):
        p = good.copy()
        p[32, 32] = v
        return p
    cases = {
        "delta": (delta, 0.5, "fewer than three"),
        "flat to the window's edge": (flat, 0.5, "lobe too wide"),
        "centre 0": (centre(0.0), 0.5, "centre"),
        "centre negative": (centre(-1.0), 0.5, "centre"),
        "centre NaN": (centre(np.nan), 0.5, "centre"),
        "centre Inf": (centre(np.inf), 0.5, "centre"),
        "a line of pixels": (line, 0.5, "singular"),
        "rising from the centre": (ring, 0.5, "positive definite"),
        "level 0": (good, 0.0, "level"),
        "level 1": (good, 1.0, "level"),
        "level NaN": (good, float("nan"), "level"),
    }
    for what, (psf, level, word) in cases.items():
        code, untouched = _raw_fit(idg, psf.shape[0], psf, level)
        assert code == -1 and untouched, what
        assert word in lib.idg_last_error().decode(), what
        if what.startswith("level"):
            continue
        with pytest.raises(idg.IdgError, match=word):
            idg.beam_fit(psf, level=level)
    for code, untouched in (_raw_fit(idg, 65, None, 0.5),
                            _raw_fit(idg, 0, good, 0.5),
                            _raw_fit(idg, 65, good, 0.5, struct_size=0),
                            _raw_fit(idg, 65, good, 0.5, struct_size=6)):
        assert code == -1 and untouched
    assert lib.idg_beam_fit(65, good.ctypes.data_as(ctypes.c_void_p), 0.5,
                            None) == -1
    assert _raw_fit(idg, 65, good, 0.5) == (0, False)
    # an older, shorter struct gets the fields it has room for
    code, _ = _raw_fit(idg, 65, good, 0.5, struct_size=32)
    assert code == 0


# ---- 4. the taps ----------------------------------------------------------------------
def _ulps(a, b):
    """Distance in float32 steps (positive finite values)."""
    return np.abs(a.view(np.int32).astype(np.int64)
                  - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("axes,R", [(AXES[0], 6), (AXES[1], 17), (AXES[2], 8),
                                    ((30.0, 20.0, 1.0), 32), (AXES[0], 0)])
def test_taps_are_the_beam(idg, axes, R):
    beam = idg.beam_from_axes(*axes)
    want_abc = rc.axes_to_abc(*axes)
    assert _error(beam[:3], want_abc) <= 1e-15
    taps = idg.beam_taps(beam, radius=R)
    assert taps.shape == (2 * R + 1, 2 * R + 1) and taps.dtype == F
    want = rc.taps_of(beam[:3], R).astype(F)
    worst = int(_ulps(taps, want).max())
    print(f"taps {axes} R {R}: worst {worst} ulp, smallest {taps.min()!r}")
    assert worst <= 1
    assert taps[R, R] == 1.0
    assert taps.max() == 1.0 and np.count_nonzero(taps == 1.0) == 1
    # a point-symmetric table
    assert np.array_equal(taps, taps[::-1, ::-1])


def test_radius_at_hand_computed_values(idg):
    """floor(sqrt(-ln(cutoff) / lambda_min)), lambda_min = 4 ln 2 / major^2.
    major 4, cutoff 1e-6: sqrt(13.8155 / 0.173287) = 8.93 -> 8; cutoff 0.1:
    sqrt(2.302585 / 0.173287) = 3.65 -> 3.  major 3 (minor 2, any angle),
    cutoff 1e-6: sqrt(13.8155 / 0.308065) = 6.70 -> 6.  major 14.3, 1e-6:
    31.9 -> 31; major 14.8: 33.04, beyond 32, refused."""
    round4 = idg.beam_from_axes(4, 4, 0)
    assert idg.beam_radius(round4) == 8
    assert idg.beam_radius(round4, cutoff=0.1) == 3
    assert idg.beam_radius(idg.beam_from_axes(3, 2, 0.5)) == 6
    assert idg.beam_radius(idg.beam_from_axes(3, 2, -1.0)) == 6
    assert idg.beam_radius(idg.beam_from_axes(14.3, 2, 0.3)) == 31
    assert idg.beam_taps(round4).shape == (17, 17)
    # the beam is still >= cutoff at that distance along the major axis, and
    # below it one pixel further
    b = idg.beam_from_axes(3, 2, 0.5)
    lam = 4 * math.log(2) / 9
    assert math.exp(-lam * 36) >= 1e-6 > math.exp(-lam * 49)
    for bad in (dict(cutoff=0.0), dict(cutoff=1.0), dict(cutoff=-1.0),
                dict(cutoff=float("nan"))):
        with pytest.raises(idg.IdgError) as e:
            idg.beam_radius(b, **bad)
        assert e.value.code == -1
    with pytest.raises(idg.IdgError, match="32"):
        idg.beam_radius(idg.beam_from_axes(14.8, 2, 0.3))
    with pytest.raises(idg.IdgError):
        idg.beam_taps(b, radius=33)
    with pytest.raises(idg.IdgError):
        idg.beam_taps(b, radius=-1)
    with pytest.raises(idg.IdgError, match="a c - b"):
        idg.beam_taps(idg.Beam(1.0, 2.0, 1.0, 0, 0, 0), radius=2)
    for bad in ((2, 3, 0), (0, 0, 0), (3, -1, 0), (3, 2, float("inf"))):
        with pytest.raises(idg.IdgError):
            idg.beam_from_axes(*bad)
    # pa is brought into (-pi/2, pi/2]: the same beam
    turned = idg.beam_from_axes(3, 2, 0.5 + math.pi)
    assert abs(turned.pa - 0.5) <= 1e-15
    assert _error(turned[:3], b[:3]) <= 1e-15
