"""The Hogbom minor cycle on the device (kernels/clean_mi355x.hip.cpp; DESIGN.md
§15) against its host twin (pinned to the contract by test_clean_host.py):
the bytes of every output, guard rows included, at every case of the host
list and at shapes with many tiles; then weigh -> psf / invert -> clean ->
predict end to end on the on-cell case."""
import json

import numpy as np
import pytest

import clean_cases as cc
import image_cases as ic
import plan_cases as pc
import weight_cases as wc
from conftest import TOLERANCE

pytestmark = pytest.mark.gpu

F = np.float32
ALL = dict(cc.CASES, **cc.LARGE)


@pytest.fixture(scope="module")
def idg():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import idg_amd
    return idg_amd


_cache = {}


def _case(idg, name):
    """The case and the buffers the host entry leaves, made once."""
    if name not in _cache:
        c = ALL[name]()
        host = cc.run_host(idg, c)
        for a in host.values():
            a.setflags(write=False)
        _cache[name] = (c, host)
    return _cache[name]


def _upload(b):
    import torch
    return dict(
        residual=torch.from_numpy(b["residual"]).cuda(),
        model=torch.from_numpy(b["model"]).cuda(),
        components=torch.from_numpy(
            b["components"].view(np.int32).reshape(-1, 3)).cuda(),
        state=torch.from_numpy(b["state"].view(np.int32).reshape(6)).cuda())


def _download(t):
    return dict(
        residual=t["residual"].cpu().numpy(), model=t["model"].cpu().numpy(),
        components=t["components"].cpu().numpy().reshape(-1).view(
            cc.COMPONENT),
        state=t["state"].cpu().numpy().view(cc.STATE))


def _run_device(idg, c, stream=None, check_every=None):
    """The case through the device entry, chunk by chunk; the buffers() as
    numpy."""
    import torch
    t = _upload(cc.buffers(c))
    psf = torch.from_numpy(c["psf"]).cuda()
    mask = None if c["mask"] is None else torch.from_numpy(c["mask"]).cuda()
    torch.cuda.synchronize()
    for n in c["chunks"]:
        out = idg.clean(t["residual"][1:-1], psf, t["model"][1:-1], mask,
                        nr_iterations=n, components=t["components"][1:-1],
                        state=t["state"], check_every=check_every,
                        stream=stream, **cc.params(c))
    assert out[0].data_ptr() == t["residual"][1:-1].data_ptr()
    if stream is not None:
        stream.synchronize()
    return _download(t)


@pytest.mark.parametrize("name", sorted(ALL))
def test_device_is_the_host(idg, name):
    c, host = _case(idg, name)
    got = _run_device(idg, c)
    st = got["state"][0]
    print(f"{name}: n_components {st['n_components']} reason {st['reason']} "
          f"peak {st['peak']!r} at {st['peak_index']}")
    assert cc.same_bytes(got, host) == []
    assert cc.guards_intact(got)


def test_large_cases_do_what_they_are_for(idg):
    c, host = _case(idg, "G2048_Gp64")
    comps, st = host["components"][1:-1], host["state"][0]
    assert st["n_components"] == 8
    assert [tuple(r)[:2] for r in comps[:3]] == [(3, 100), (2047, 2040),
                                                 (8, 256)]
    for name in ("G256_Gp256", "G256_Gp32"):
        c, host = _case(idg, name)
        assert host["state"][0]["n_components"] == 40
        # components in several tiles (8 rows each), some tiles more than once
        rows = [int(r["y"]) // 8 for r in host["components"][1:-1]]
        assert 4 <= len(set(rows)) < len(rows)


@pytest.mark.parametrize("name", ["G256_Gp32", "three_calls_of_5",
                                  "mask_hides_the_maximum"])
def test_same_bytes_again_and_on_a_stream(idg, name):
    import torch
    c, host = _case(idg, name)
    assert cc.same_bytes(_run_device(idg, c), host) == []
    stream = torch.cuda.Stream()
    got = _run_device(idg, c, stream=stream)
    assert cc.same_bytes(got, host) == []
    idg.release_workspaces(stream)


@pytest.mark.parametrize("name", ["G256_Gp32", "G2048_Gp64", "G65_Gp16_odd_G"])
def test_same_bytes_with_every_tile_rescanning(idg, name, monkeypatch):
    c, host = _case(idg, name)
    monkeypatch.setenv("IDG_CLEAN_RESCAN", "1")
    assert cc.same_bytes(_run_device(idg, c), host) == []


@pytest.mark.parametrize("name", ["G256_Gp32", "threshold_reached",
                                  "components_full", "three_calls_of_5"])
def test_check_every_4_is_check_every_none(idg, name):
    c, host = _case(idg, name)
    assert cc.same_bytes(_run_device(idg, c, check_every=4), host) == []


def test_unaligned_planes_take_the_scalar_path(idg):
    """A residual that starts 4 bytes off a 16-byte boundary (G % 4 == 0, so
    only the pointer rules out the float4 path): the same bytes."""
    import torch
    c, host = _case(idg, "G40_Gp40")
    G = c["G"]
    flat = torch.zeros(G * G + 1, dtype=torch.float32, device="cuda")
    res = flat[1:].view(G, G)
    assert res.data_ptr() % 16 == 4
    res.copy_(torch.from_numpy(c["residual"]))
    _, model, comps, state = idg.clean(
        res, torch.from_numpy(c["psf"]).cuda(), nr_iterations=25,
        **cc.params(c))
    assert res.cpu().numpy().tobytes() == host["residual"][1:-1].tobytes()
    assert model.cpu().numpy().tobytes() == host["model"][1:-1].tobytes()
    assert (state.cpu().numpy().tobytes() == host["state"].tobytes())
    assert (comps.cpu().numpy().tobytes()
            == host["components"][1:-1].tobytes())


def test_invalid_arguments_leave_the_buffers(idg):
    import torch
    c, _ = _case(idg, "G40_Gp40")
    before = cc.buffers(c)
    t = _upload(before)
    psf = torch.from_numpy(c["psf"]).cuda()
    args = (t["residual"][1:-1], psf, t["model"][1:-1])
    kw = dict(components=t["components"][1:-1], state=t["state"],
              **cc.params(c))
    for bad in (dict(gain=float("nan")), dict(threshold=-1.0),
                dict(cycle_fraction=float("inf")), dict(nr_iterations=-1),
                dict(max_components=-1)):
        with pytest.raises(idg.IdgError) as e:
            idg.clean(*args, **dict(kw, **bad))
        assert e.value.code == -1
    with pytest.raises(idg.IdgError):
        idg.clean(t["residual"][1:-1], torch.zeros((41, 41), device="cuda"),
                  t["model"][1:-1], **kw)
    torch.cuda.synchronize()
    assert cc.same_bytes(_download(t), before) == []
    # a state the device cannot refuse: no iteration runs on it
    t["state"][0] = 26
    idg.clean(*args, **kw)
    got = _download(t)
    assert got["state"][0]["n_components"] == 26
    assert got["state"][0]["peak"] == np.abs(c["residual"]).max()
    for k in ("residual", "model", "components"):
        assert got[k].tobytes() == before[k].tobytes()


# ---- end to end on the on-cell case ----------------------------------------------
def _pairs(z):
    import torch
    return torch.from_numpy(np.ascontiguousarray(
        np.stack([z.real, z.imag], axis=-1).astype(F))).cuda()


def test_a_point_source_through_the_chain(idg):
    """weigh (natural) -> psf -> invert(sum_weights=) -> stokes_i -> clean
    (gain 1, one iteration, Gp = G) -> predict on weight_cases.oncell(): taper
    1 and samples on cell centres, so every step is exact up to rounding.

    The dirty image, the PSF and the component are each within TOLERANCE of
    the same exact quantity (the existing PSF and invert tests meet it at
    1.6-2.8e-6 and 3-4e-8), and the residual is a sum of three such
    differences: hence the factor 3, derived, not measured; the predicted
    visibilities alike."""
    import torch
    c = wc.oncell()
    G, S, st = c["G"], c["S"], c["case"]["nr_stations"]
    flux, py, px = 2.5, G // 2 + 3, G // 2 - 5
    host = dict(c["case"], geom=dict(pc.ONCELL, C=1), md=c["md"], W=1,
                w_step=0.0)
    sky = np.zeros((4, G, G), complex)
    sky[0, py, px] = sky[3, py, px] = flux
    vis_in = ic.direct_predict(host, sky)
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda()
         for k in ("uvw", "wn", "weights")}
    t["vis"] = _pairs(vis_in)
    t["md"] = torch.from_numpy(c["md"].view(np.int32).reshape(-1, 9)).cuda()
    sph = torch.from_numpy(c["case"]["spheroidal"]).cuda()
    aterms = torch.from_numpy(c["case"]["aterms"]).cuda()
    ns = c["md"].size

    iw, wvis, total, density, ab = idg.weigh(
        G, S, c["image_size"], t["uvw"], t["wn"], t["weights"], t["md"],
        t["vis"])
    beam = idg.psf(G, S, c["image_size"], 0.0, st, t["uvw"], t["wn"],
                   t["weights"], sph, t["md"])
    dirty = idg.invert(ns, G, S, c["image_size"], 0.0, 1, st, t["uvw"],
                       t["wn"], wvis, sph, aterms, t["md"], sum_weights=total)
    residual, model, comps, state = idg.clean(
        idg.stokes_i(dirty), idg.stokes_i(beam), gain=1.0, nr_iterations=1,
        max_components=1)
    rec = comps.cpu().numpy().reshape(-1).view(cc.COMPONENT)[0]
    res = residual.cpu().numpy()
    oy, ox = py - G // 2, px - G // 2
    patch = res[max(oy, 0):min(oy + G, G), max(ox, 0):min(ox + G, G)]
    assert patch.size == (G - 3) * (G - 5)

    vis_out = torch.zeros_like(t["vis"])
    idg.predict(ns, G, S, c["image_size"], 0.0, 1, st, t["uvw"], t["wn"],
                vis_out, sph, aterms, t["md"], idg.model_image(model))
    rows = ic.covered_rows(host)
    out = vis_out.cpu().numpy()
    out = out[..., 0].astype(np.float64) + 1j * out[..., 1]
    figures = {
        "component_at": [int(rec["y"]), int(rec["x"])],
        "component_error_over_flux": float(abs(rec["value"] - flux) / flux),
        "residual_max_over_flux": float(np.abs(patch).max() / flux),
        "predict_max_abs_over_flux": float(
            np.abs(out[rows] - vis_in[rows]).max() / flux),
        "tolerance": TOLERANCE,
    }
    print("clean parity: " + json.dumps(figures))
    assert figures["component_at"] == [py, px]
    assert int(state.cpu()[0]) == 1 and rows.sum() > 0
    assert figures["component_error_over_flux"] <= TOLERANCE
    assert figures["residual_max_over_flux"] <= 3 * TOLERANCE
    assert figures["predict_max_abs_over_flux"] <= 3 * TOLERANCE
