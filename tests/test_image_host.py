"""Grid <-> image on the host: idg_taper_to_image, and the
conventions of grid_to_image / image_to_grid -- the FFT's sign, the centre
flips with no further ramp, the 1/S^2, the sign of the w-layer phasor --
derived by composing their float64 restatement (tests/image_cases.py) with
the C oracle and pipeline_oracle and comparing with the contract's direct
sums.  No device needed."""
import json
import os

import numpy as np
import pytest

import image_cases as ic
import pipeline_oracle as pl
from conftest import REPO

PARITY = json.load(open(os.path.join(REPO, "profiles", "image",
                                     "parity.json")))
# (nr_w_layers, w_step_in_lambda): w = 0 on one layer; w over three layers
LAYERS = [(1, 0.0), (3, 60.0)]


@pytest.fixture(scope="module")
def idg():
    import idg_amd
    return idg_amd


@pytest.fixture(scope="module", params=LAYERS, ids=["W1", "W3"])
def case(request):
    W, w_step = request.param
    c = ic.small_case(W, w_step)
    c["correction"], c["mask"] = ic.correction_for(c)
    return c


# ---- taper_to_image ---------------------------------------------------------
def interpolant(S, G, taper):
    """The definition: the taper's S x S samples at a_p = p + 0.5 - S/2 as a
    trigonometric polynomial of period S, frequencies |k| < S/2 whole and the
    Nyquist pair as one cosine, evaluated at a_j = (j - G/2) S / G."""
    a_p = np.arange(S) + 0.5 - S // 2
    a_j = (np.arange(G) - G // 2) * S / G
    delta = a_j[:, None] - a_p[None, :]
    k = np.arange(1, (S + 1) // 2)
    d = 1.0 + 2.0 * np.cos(2 * np.pi * k[None, None, :] * delta[..., None]
                           / S).sum(axis=-1)
    if S % 2 == 0:
        d = d + np.cos(np.pi * delta)
    d /= S
    return d @ taper.astype(np.float64) @ d.T


@pytest.mark.parametrize("S,G", [(32, 128), (16, 128), (24, 64), (8, 100),
                                 (7, 64)])
def test_taper_equals_its_definition(idg, S, G):
    rng = np.random.default_rng(S)
    taper = rng.uniform(0.1, 1.0, (S, S)).astype(np.float32)
    got = idg.taper_to_image(S, G, taper)
    want = interpolant(S, G, taper)
    assert got.dtype == np.float64 and got.shape == (G, G)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("S,G", [(32, 128), (16, 128)])
def test_taper_reproduces_its_samples(idg, S, G):
    """G / S even: image pixel (p + 0.5 - S/2) G / S + G/2 is sample p."""
    taper = ic.kaiser_taper(S)
    got = idg.taper_to_image(S, G, taper)
    r = G // S
    at = (np.arange(S) * r + r // 2 + G // 2 - (S // 2) * r)
    assert np.all((0 <= at) & (at < G))
    assert np.abs(got[np.ix_(at, at)] - taper).max() <= 1e-12


def test_taper_of_a_symmetric_taper_is_real_and_symmetric(idg):
    S, G = 32, 128
    got = idg.taper_to_image(S, G, ic.kaiser_taper(S))
    assert np.isrealobj(got) and np.all(np.isfinite(got))
    # sample p mirrors to S - 1 - p about a = 0, pixel j to G - j about G/2
    inner = got[1:, 1:]
    assert np.abs(inner - inner[::-1, :]).max() <= 1e-13
    assert np.abs(inner - inner[:, ::-1]).max() <= 1e-13
    assert np.abs(got - got.T).max() <= 1e-13


def test_taper_invalid_sizes(idg):
    import ctypes
    from idg_amd._lib import lib
    sph = np.ones((4, 4), np.float32)
    out = np.zeros((8, 8), np.float64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.idg_taper_to_image(4, 8, p(sph), p(out)) == 0
    for S, G in ((0, 8), (-1, 8), (4, 0), (4, -3)):
        assert lib.idg_taper_to_image(S, G, p(sph), p(out)) == -1
        assert b"idg_taper_to_image" in lib.idg_last_error()
    assert lib.idg_taper_to_image(4, 8, None, p(out)) == -1
    assert lib.idg_taper_to_image(4, 8, p(sph), None) == -1
    with pytest.raises(ValueError):
        idg.taper_to_image(8, 16, sph)


# ---- conventions ------------------------------------------------------------
def test_restatement_is_an_adjoint_pair():
    """<image_to_grid(I), Gamma> = <I, grid_to_image(Gamma)> in float64."""
    rng = np.random.default_rng(0)
    G, W = 64, 3
    cplx = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)
    image, grid = cplx(4, G, G), cplx(W, 4, G, G)
    corr = rng.uniform(0.5, 2.0, (G, G))
    a = np.vdot(ic.image_to_grid(image, W, 0.3, 700.0, corr), grid)
    b = np.vdot(image, ic.grid_to_image(grid, 0.3, 700.0, corr))
    assert abs(a - b) <= 1e-12 * abs(a)


def test_invert_against_the_direct_sum(oracle_lib, case):
    """Random visibilities, identity A-terms: oracle gridder -> FFT -> adder
    -> grid_to_image(correction / S^2) is the contract's sum, to the
    algorithm's own error (profiles/image/parity.json)."""
    got = ic.chain_invert(oracle_lib, case, case["vis"], case["correction"],
                          ic.identity_aterms(case))
    want = ic.direct_invert(case, pl.to_complex(case["vis"])) * case["mask"]
    err = ic.rel_max(got, want)
    recorded = PARITY[f"invert_W{case['W']}"]
    print(f"invert W = {case['W']}: {err:.3e} of the peak "
          f"(recorded {recorded:.3e})")
    assert recorded < 1e-2
    assert err <= 2 * recorded


def test_unit_visibility_images_to_modulus_one(oracle_lib, case):
    vis = np.zeros_like(case["vis"])
    row = int(case["md"]["time_offset"][1]) + 3
    vis[row, 0, 0, 0] = 1.0
    got = ic.chain_invert(oracle_lib, case, vis, case["correction"],
                          ic.identity_aterms(case))
    inside = np.abs(got[0])[case["mask"]]
    assert np.abs(inside - 1.0).max() < 1e-2
    assert np.abs(got[1:]).max() < 1e-6


def test_predict_against_the_direct_sum(oracle_lib, case):
    """A few off-centre point sources inside the imaged field."""
    G = ic.SMALL["G"]
    image = np.zeros((4, G, G), complex)
    for (y, x), v in (((40, 50), 1.0), ((85, 34), 0.7j), ((64, 93), -0.5)):
        assert case["mask"][y, x]
        image[0, y, x] = v
        image[3, y, x] = 0.5 * v
        image[1, y, x] = 0.25j * v
    got = ic.chain_predict(oracle_lib, case, image, case["correction"],
                           ic.identity_aterms(case))
    want = ic.direct_predict(case, image)
    err = ic.rel_max(got, want)
    recorded = PARITY[f"predict_W{case['W']}"]
    print(f"predict W = {case['W']}: {err:.3e} of the peak "
          f"(recorded {recorded:.3e})")
    assert recorded < 1e-2
    assert err <= 2 * recorded
    one = np.zeros((4, G, G), complex)
    one[0, 40, 50] = 1.0
    v = ic.chain_predict(oracle_lib, case, one, case["correction"],
                         ic.identity_aterms(case))
    rows = ic.covered_rows(case)
    assert np.abs(np.abs(v[rows, :, 0]) - 1.0).max() < 1e-2


def test_adjointness_of_the_chain(oracle_lib, case):
    """<predict(I), V> = <I, invert(V)> with the case's own (non-identity)
    A-terms: the float64 steps are exact adjoints, the residue is the f32
    oracle's rounding."""
    rng = np.random.default_rng(1)
    G = ic.SMALL["G"]
    image = rng.normal(size=(4, G, G)) + 1j * rng.normal(size=(4, G, G))
    vis = pl.to_complex(case["vis"]) * ic.covered_rows(case)[:, None, None]
    a = np.vdot(vis, ic.chain_predict(oracle_lib, case, image,
                                      case["correction"]))
    b = np.vdot(ic.chain_invert(oracle_lib, case, case["vis"],
                                case["correction"]), image)
    print(f"adjointness W = {case['W']}: {abs(a - b) / abs(a):.3e}")
    assert abs(a - b) <= 1e-5 * abs(a)
