"""The mirror path's single B fragment (run on the GPU box: -m gpu).

On mirror subgrids (w = 0, even S) the gridder builds one B fragment per
K-step, Bc = (V.re | V.im), runs the cos and the sin GEMM against it and maps
the sin tiles Y' = s * Bc to Y = s * Bs in the epilogue (Y.re = -Y'.im, Y.im =
Y'.re); a fill holds 64 K-steps (64 timesteps at C = 16).  Every case: 3
stations, 1 timeslot (3 subgrids), w = 0, through both launch forms, against
the oracle in the scale-free per-subgrid RMS with the harness tolerance.
"""
import numpy as np
import pytest

from conftest import TOLERANCE

pytestmark = pytest.mark.gpu

FORMS = ["split", "combined"]
# timesteps per fill at C = 16, and a fill's K-step capacity
F, K = 64, 64


@pytest.fixture(scope="module")
def idg():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import idg_amd
    return idg_amd


def _rel_rms(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-300)))


def _params(p):
    return (p["nr_subgrids"], p["grid_size"], p["subgrid_size"],
            p["image_size"], p["w_step_in_lambda"], p["nr_channels"],
            p["nr_stations"])


_cases = {}


def _case(idg, oracle_lib, key, T, C, S, edit):
    """Inputs and the oracle's subgrids of one case, computed once and shared
    by the launch forms."""
    if key not in _cases:
        st, ts, G = 3, 1, 1024
        a = idg.generate(st, ts, T, C, G, S)
        assert not a["uvw"][..., 2].any()  # w = 0: the mirror path
        edit(a["visibilities"])
        p = dict(nr_subgrids=idg.nr_subgrids_for(st, ts), grid_size=G,
                 subgrid_size=S, image_size=idg.IMAGE_SIZE,
                 w_step_in_lambda=0.0, nr_channels=C, nr_stations=st)
        go = np.zeros((p["nr_subgrids"], 4, S, S, 2), np.float32)
        oracle_lib.gridder(*_params(p), a["uvw"], a["wavenumbers"],
                           a["visibilities"], a["spheroidal"], a["aterms"],
                           a["metadata"], go)
        go.setflags(write=False)
        _cases[key] = (p, a, go)
    return _cases[key]


def _check(idg, case, tag):
    p, a, go = case
    g = np.zeros_like(go)
    idg.c_run_gridder(*_params(p), a["uvw"], a["wavenumbers"],
                      a["visibilities"], a["spheroidal"], a["aterms"],
                      a["metadata"], g)
    assert np.isfinite(g).all()
    errs = [_rel_rms(g[s], go[s]) for s in range(g.shape[0])]
    print(tag, " ".join(f"{e:.2e}" for e in errs))
    for s, e in enumerate(errs):
        assert e <= TOLERANCE, (tag, s, e)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("S,comp", [(32, k) for k in range(8)] + [(64, 3)])
def test_one_visibility_component_at_a_time(idg, oracle_lib, monkeypatch, S,
                                            comp, form):
    # all visibilities zero but one of the 8 real components (random per
    # timestep and channel): a wrong column swap or sign in the epilogue's
    # Y' -> Y map is an O(1) error in a known correlation
    monkeypatch.setenv("IDG_KERNEL_FORM", form)

    def edit(vis):
        rng = np.random.default_rng(100 + comp)
        vis[:] = 0.0
        vis.reshape(vis.shape[:3] + (8,))[..., comp] = rng.uniform(
            -1.0, 1.0, vis.shape[:3])

    _check(idg, _case(idg, oracle_lib, ("comp", S, comp), 8, 4, S, edit),
           f"component {comp} S={S} {form}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("T,C", [
    (F, 16), (F + 4, 16), (2 * F + 2, 16),  # one fill, a short and a third one
    (2 * F + 2, 6),            # ragged channel quad
    (40, 256),                 # blocked summation: one flush, then more fills
    (8, 4 * K + 4),            # a second channel fill of one quad
])
def test_fill_boundaries(idg, oracle_lib, monkeypatch, T, C, form):
    monkeypatch.setenv("IDG_KERNEL_FORM", form)
    _check(idg, _case(idg, oracle_lib, ("fill", T, C), T, C, 32,
                      lambda vis: None), f"fill T={T} C={C} {form}")


@pytest.mark.parametrize("form", FORMS)
def test_rescale_with_the_sin_tiles_live(idg, oracle_lib, monkeypatch, form):
    # a 1e6 burst that starts exactly at the second fill: the sums so far,
    # the Y' tiles among them, are rescaled and the fill is split again
    monkeypatch.setenv("IDG_KERNEL_FORM", form)

    def edit(vis):
        vis[:, F:] *= np.float32(1e6)

    _check(idg, _case(idg, oracle_lib, "late_burst", F + 8, 16, 32, edit),
           f"late_burst {form}")


@pytest.mark.parametrize("form", FORMS)
def test_burst_in_the_unscanned_half_of_the_first_fill(idg, oracle_lib,
                                                       monkeypatch, form):
    # the prologue's max-|V| pass covers the first 32 timesteps at C = 16,
    # half of the first fill: a 1e6 burst confined to timesteps 32..63 makes
    # the first fill itself split again, the scale already set and the sums
    # still zero
    monkeypatch.setenv("IDG_KERNEL_FORM", form)

    def edit(vis):
        vis[:, F // 2:F] *= np.float32(1e6)

    _check(idg, _case(idg, oracle_lib, "first_fill_burst", F + 8, 16, 32,
                      edit), f"first_fill_burst {form}")
