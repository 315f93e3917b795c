"""Clark CLEAN on the device (kernels/clark_mi355x.hip.cpp)
against its host twin (pinned to the contract by test_clark_host.py): the
bytes of every output, guard rows included, at every case of the host list,
at shapes with many tiles and at every form of the cycle kernel; then weigh ->
psf / invert -> clark -> predict end to end on the on-cell case.  (The
candidate list is not exposed, and the cycle kernel reads its PSF from one
place only: global memory.)"""
import json

import numpy as np
import pytest

import clark_cases as kc
import image_cases as ic
import plan_cases as pc
import weight_cases as wc
from conftest import TOLERANCE

pytestmark = pytest.mark.gpu

F = np.float32
ALL = dict(kc.CASES, **kc.LARGE)


@pytest.fixture(scope="module")
def idg():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import idg_amd
    return idg_amd


_cache = {}


def _case(idg, name, **edit):
    """The case and the buffers the host entry leaves, made once."""
    key = (name, tuple(sorted(edit.items())))
    if key not in _cache:
        c = dict(ALL[name](), **edit)
        host = kc.run_host(idg, c)
        for a in host.values():
            a.setflags(write=False)
        _cache[key] = (c, host)
    return _cache[key]


def _upload(b):
    import torch
    return dict(
        residual=torch.from_numpy(b["residual"]).cuda(),
        model=torch.from_numpy(b["model"]).cuda(),
        components=torch.from_numpy(
            b["components"].view(np.int32).reshape(-1, 3)).cuda(),
        state=torch.from_numpy(b["state"].view(np.int32).reshape(9)).cuda())


def _download(t):
    return dict(
        residual=t["residual"].cpu().numpy(), model=t["model"].cpu().numpy(),
        components=t["components"].cpu().numpy().reshape(-1).view(
            kc.COMPONENT),
        state=t["state"].cpu().numpy().view(kc.STATE))


def _run_device(idg, c, stream=None, check_every=None, chunks=None):
    """The case through the device entry, call by call; the buffers() as
    numpy."""
    import torch
    t = _upload(kc.buffers(c))
    psf = torch.from_numpy(c["psf"]).cuda()
    mask = None if c["mask"] is None else torch.from_numpy(c["mask"]).cuda()
    torch.cuda.synchronize()
    for n in c["chunks"] if chunks is None else chunks:
        out = idg.clark(t["residual"][1:-1], psf, t["model"][1:-1], mask,
                        nr_rounds=n, components=t["components"][1:-1],
                        state=t["state"], check_every=check_every,
                        stream=stream, **kc.params(c))
    assert out[0].data_ptr() == t["residual"][1:-1].data_ptr()
    if stream is not None:
        stream.synchronize()
    return _download(t)


@pytest.mark.parametrize("name", sorted(ALL))
def test_device_is_the_host(idg, name):
    c, host = _case(idg, name)
    got = _run_device(idg, c)
    st = got["state"][0]
    print(f"{name}: " + ", ".join(f"{k} {st[k]!r}" for k in kc.STATE.names))
    assert kc.same_bytes(got, host) == []
    assert kc.guards_intact(got)


def test_large_cases_do_what_they_are_for(idg):
    c, host = _case(idg, "G2048_Gp64")
    comps, st = host["components"][1:-1], host["state"][0]
    assert {(int(y), int(x)) for y, x, _ in comps[:st["n_components"]]} == {
        (3, 100), (2047, 2040), (8, 256)}
    _, host = _case(idg, "G256_full_list", chunks=(1,))
    st = host["state"][0]
    # every thread of the cycle kernel holds sixteen entries, or nearly
    assert 15 * 1024 < st["n_candidates"] <= 16384 and st["n_components"] > 0
    for name in ("G300_Gp64", "G258_Gp33_scalar"):
        _, host = _case(idg, name)
        st = host["state"][0]
        cols = {int(r["x"]) // 256
                for r in host["components"][1:-1][:st["n_components"]]}
        assert cols == {0, 1} and st["n_components"] > 100


@pytest.mark.parametrize("max_candidates", [1000, 2048, 8192, 16384])
def test_every_form_of_the_cycle_kernel(idg, max_candidates):
    """`many` has some 7,900 qualifying pixels: under 1,000 and 2,048 (and
    the case's own 4,096) the histogram bounds the list (1, 2 and 4 entries a
    thread), under 8,192 and 16,384 it does not (8 and 16 entries, the upper
    ones empty)."""
    c, host = _case(idg, "many", max_candidates=max_candidates)
    _, first = _case(idg, "many", max_candidates=max_candidates, chunks=(1,))
    n = first["state"][0]["n_candidates"]
    assert (n <= max_candidates) and (n > 1024) == (max_candidates > 1024)
    assert kc.same_bytes(_run_device(idg, c), host) == []


@pytest.mark.parametrize("name", ["G300_Gp64", "two_calls_of_three",
                                  "mask_hides_the_peak"])
def test_same_bytes_again_and_on_a_stream(idg, name):
    import torch
    c, host = _case(idg, name)
    assert kc.same_bytes(_run_device(idg, c), host) == []
    stream = torch.cuda.Stream()
    got = _run_device(idg, c, stream=stream)
    assert kc.same_bytes(got, host) == []
    # the workspace of that stream again, then released
    assert kc.same_bytes(_run_device(idg, c, stream=stream), host) == []
    idg.release_workspaces(stream)


@pytest.mark.parametrize("name", ["G300_Gp64", "low", "flat",
                                  "components_full_mid_round",
                                  "three_iterations_per_round"])
def test_check_every_is_check_every_none(idg, name):
    c, host = _case(idg, name)
    assert kc.same_bytes(_run_device(idg, c, check_every=1), host) == []
    assert kc.same_bytes(_run_device(idg, c, check_every=2), host) == []


def test_all_rounds_by_default(idg):
    """nr_rounds=None on the device: a round at a time until the reason read
    back is set."""
    c, host = _case(idg, "low")
    assert host["state"][0]["reason"] == 1
    got = _run_device(idg, c, chunks=(None,))
    assert kc.same_bytes(got, host) == []


def test_unaligned_planes_take_the_scalar_path(idg):
    """A residual that starts 4 bytes off a 16-byte boundary (G % 4 == 0, so
    only the pointer rules out the float4 path): the same bytes."""
    import torch
    c, host = _case(idg, "low")
    G = c["G"]
    flat = torch.zeros(G * G + 1, dtype=torch.float32, device="cuda")
    res = flat[1:].view(G, G)
    assert res.data_ptr() % 16 == 4
    res.copy_(torch.from_numpy(c["residual"]))
    _, model, comps, state = idg.clark(
        res, torch.from_numpy(c["psf"]).cuda(), nr_rounds=6, **kc.params(c))
    assert res.cpu().numpy().tobytes() == host["residual"][1:-1].tobytes()
    assert model.cpu().numpy().tobytes() == host["model"][1:-1].tobytes()
    assert state.cpu().numpy().tobytes() == host["state"].tobytes()
    assert (comps.cpu().numpy().tobytes()
            == host["components"][1:-1].tobytes())


def test_invalid_arguments_leave_the_buffers(idg):
    import torch
    c, _ = _case(idg, "low")
    before = kc.buffers(c)
    t = _upload(before)
    psf = torch.from_numpy(c["psf"]).cuda()
    args = (t["residual"][1:-1], psf, t["model"][1:-1])
    kw = dict(components=t["components"][1:-1], state=t["state"],
              nr_rounds=2, **kc.params(c))
    for bad in (dict(gain=float("nan")), dict(threshold=-1.0),
                dict(cycle_fraction=float("inf")), dict(nr_rounds=-1),
                dict(iterations_per_round=-1), dict(max_components=-1),
                dict(select_fraction=1.5), dict(select_fraction=float("nan")),
                dict(max_candidates=0), dict(max_candidates=16385)):
        with pytest.raises(idg.IdgError) as e:
            idg.clark(*args, **dict(kw, **bad))
        assert e.value.code == -1
    with pytest.raises(idg.IdgError):
        idg.clark(t["residual"][1:-1], torch.zeros((97, 97), device="cuda"),
                  t["model"][1:-1], **kw)
    torch.cuda.synchronize()
    assert kc.same_bytes(_download(t), before) == []
    # a state the device cannot refuse: no round runs on it
    t["state"][0] = 1001
    idg.clark(*args, **kw)
    got = _download(t)
    st = got["state"][0]
    assert (st["n_components"], st["rounds"], st["reason"]) == (1001, 0, 0)
    assert st["peak"] == np.abs(c["residual"]).max()
    for k in ("residual", "model", "components"):
        assert got[k].tobytes() == before[k].tobytes()


# ---- end to end on the on-cell case ----------------------------------------------
def _pairs(z):
    import torch
    return torch.from_numpy(np.ascontiguousarray(
        np.stack([z.real, z.imag], axis=-1).astype(F))).cuda()


def test_a_point_source_through_the_chain(idg):
    """weigh (natural) -> psf -> invert(sum_weights=) -> stokes_i -> clark
    (gain 1, one round of one iteration, Gp = G) -> predict on
    weight_cases.oncell(), as test_gpu_clean.py does with clean and with that
    test's bars: the dirty image, the PSF and the component are each within
    TOLERANCE of the same exact quantity, and the residual is a sum of three
    such differences: hence the factor 3, derived, not measured; the
    predicted visibilities alike."""
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
    residual, model, comps, state = idg.clark(
        idg.stokes_i(dirty), idg.stokes_i(beam), gain=1.0, nr_rounds=1,
        iterations_per_round=1, max_components=1)
    rec = comps.cpu().numpy().reshape(-1).view(kc.COMPONENT)[0]
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
    print("clark parity: " + json.dumps(figures))
    assert figures["component_at"] == [py, px]
    assert int(state.cpu()[0]) == 1 and rows.sum() > 0
    assert figures["component_error_over_flux"] <= TOLERANCE
    assert figures["residual_max_over_flux"] <= 3 * TOLERANCE
    assert figures["predict_max_abs_over_flux"] <= 3 * TOLERANCE
