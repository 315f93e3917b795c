"""The restore step on the device (kernels/restore_mi355x.hip.cpp; DESIGN.md
§16) against its host twin (pinned to the contract by test_restore_host.py):
the bytes of the restored plane, guard rows included, at every case of the
host list and at shapes with many tiles; then weigh -> psf / invert -> clean
-> restore end to end on the on-cell case."""
import json

import numpy as np
import pytest

import clean_cases as cc
import image_cases as ic
import plan_cases as pc
import restore_cases as rc
import weight_cases as wc
from conftest import TOLERANCE

pytestmark = pytest.mark.gpu

F = np.float32
ALL = dict(rc.CASES, **rc.LARGE)


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
        host = rc.run_host(idg, c)
        for a in host.values():
            a.setflags(write=False)
        _cache[name] = (c, host)
    return _cache[name]


def _run_device(idg, c, stream=None, residual=True, alias=None):
    """The case through the device entry; the buffers() as numpy.  residual
    = False drops the case's residual, alias overrides the case's choice."""
    import torch
    c = dict(c)
    if not residual:
        c["residual"] = None
    if alias is not None:
        c["alias"] = alias and c["residual"] is not None
    b = rc.buffers(c)
    t = {k: torch.from_numpy(v).cuda() for k, v in b.items()
         if not (k == "restored" and c["alias"])}
    if c["alias"]:
        t["restored"] = t["residual"]
    taps = torch.from_numpy(c["taps"]).cuda()
    torch.cuda.synchronize()
    out = idg.restore(t["model"][1:-1],
                      t["residual"][1:-1] if "residual" in t else None,
                      taps=taps, out=t["restored"][1:-1], stream=stream)
    assert out.data_ptr() == t["restored"][1:-1].data_ptr()
    if stream is not None:
        stream.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def _host_variant(idg, c, residual=True, alias=None):
    c = dict(c)
    if not residual:
        c["residual"] = None
    if alias is not None:
        c["alias"] = alias and c["residual"] is not None
    return rc.run_host(idg, c)


@pytest.mark.parametrize("name", sorted(ALL))
def test_device_is_the_host(idg, name):
    c, host = _case(idg, name)
    got = _run_device(idg, c)
    assert rc.same_bytes(got, host) == []
    assert rc.guards_intact(got)


@pytest.mark.parametrize("name", sorted(ALL))
def test_same_bytes_on_a_second_stream(idg, name):
    import torch
    c, host = _case(idg, name)
    stream = torch.cuda.Stream()
    got = _run_device(idg, c, stream=stream)
    assert rc.same_bytes(got, host) == []
    assert rc.guards_intact(got)


@pytest.mark.parametrize("name", sorted(ALL))
@pytest.mark.parametrize("residual,alias", [(False, False), (True, True),
                                            (True, False)])
def test_with_and_without_residual_aliased_and_not(idg, name, residual,
                                                   alias):
    c, _ = _case(idg, name)
    if c["residual"] is None and residual:
        c = dict(c, residual=np.random.default_rng(5).normal(
            size=(c["G"], c["G"])).astype(F))
    host = _host_variant(idg, c, residual, alias)
    got = _run_device(idg, c, residual=residual, alias=alias)
    assert sorted(got) == sorted(host)
    assert rc.same_bytes(got, host) == []
    assert rc.guards_intact(got)


def test_seam_cases_do_what_they_are_for(idg):
    for name in rc.LARGE:
        c, _ = _case(idg, name)
        G, R, m = c["G"], c["R"], c["model"]
        assert G // rc.TILE_COLS >= 3 and G % rc.TILE_COLS
        assert G // rc.TILE_ROWS >= 3 and G % rc.TILE_ROWS
        for s in range(rc.TILE_COLS, G, rc.TILE_COLS):
            assert m[:, s - 1].any() and m[:, s].any()
        for s in range(rc.TILE_ROWS, G, rc.TILE_ROWS):
            assert m[s - 1].any() and m[s].any()
        # the whole haloed window of tile (1, 1) is non-zero: every round of
        # its scan fills the list, and there are several
        window = m[rc.TILE_ROWS - R:2 * rc.TILE_ROWS + R,
                   rc.TILE_COLS - R:2 * rc.TILE_COLS + R]
        assert window.all() and window.size > 2 * 1024
    assert rc.LARGE["G200_R4_tile_seams"]()["G"] % 4 == 0
    assert rc.LARGE["G203_R4_tile_seams_scalar"]()["G"] % 4 != 0


def test_unaligned_model_takes_the_scalar_scan(idg):
    """A model that starts 4 bytes off a 16-byte boundary (G % 4 == 0, so only
    the pointer rules out the float4 scan): the same bytes."""
    import torch
    c, host = _case(idg, "G200_R4_tile_seams")
    G = c["G"]
    flat = torch.zeros(G * G + 1, dtype=torch.float32, device="cuda")
    model = flat[1:].view(G, G)
    assert model.data_ptr() % 16 == 4
    model.copy_(torch.from_numpy(c["model"]))
    out = idg.restore(model, torch.from_numpy(c["residual"]).cuda(),
                      taps=torch.from_numpy(c["taps"]).cuda())
    assert out.cpu().numpy().tobytes() == host["restored"][1:-1].tobytes()


def test_beam_argument_uploads_the_host_taps(idg):
    import torch
    c, _ = _case(idg, "G37_R3_scalar_path")
    beam = idg.beam_from_axes(3, 2, 0.5)
    want = idg.restore(c["model"], c["residual"], beam=beam)
    stream = torch.cuda.Stream()
    model = torch.from_numpy(c["model"]).cuda()
    residual = torch.from_numpy(c["residual"]).cuda()
    torch.cuda.synchronize()
    got = idg.restore(model, residual, beam=beam, stream=stream)
    stream.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes()
    # and beam_fit on a device psf is beam_fit on the host's copy of it
    psf = rc.gaussian_psf(200, rc.axes_to_abc(3.0, 2.0, 0.5))
    assert idg.beam_fit(torch.from_numpy(psf).cuda()) == idg.beam_fit(psf)
    small = rc.gaussian_psf(12, rc.axes_to_abc(3.0, 2.0, 0.5))
    assert idg.beam_fit(torch.from_numpy(small).cuda()) == idg.beam_fit(small)


def test_invalid_arguments_leave_the_buffers(idg):
    import torch
    c, _ = _case(idg, "G37_R3_scalar_path")
    b = rc.buffers(c)
    t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    taps = torch.from_numpy(c["taps"]).cuda()
    m, r, o = t["model"][1:-1], t["residual"][1:-1], t["restored"][1:-1]
    G = c["G"]
    inside = t["residual"].view(-1)[G + 4:G + 4 + G * G].view(G, G)
    big = torch.zeros((67, 67), dtype=torch.float32, device="cuda")
    for bad in (dict(model=m, residual=r, taps=taps, out=m),
                dict(model=m, residual=m, taps=taps, out=o),
                dict(model=m, residual=r, taps=taps, out=inside),
                dict(model=m, residual=r, taps=big, out=o)):
        with pytest.raises(idg.IdgError) as e:
            idg.restore(**bad)
        assert e.value.code == -1
    torch.cuda.synchronize()
    for k in b:
        assert t[k].cpu().numpy().tobytes() == b[k].tobytes()


# ---- end to end on the on-cell case ----------------------------------------------
def _pairs(z):
    import torch
    return torch.from_numpy(np.ascontiguousarray(
        np.stack([z.real, z.imag], axis=-1).astype(F))).cuda()


def test_a_point_source_through_the_chain(idg):
    """weigh (natural) -> psf -> invert(sum_weights=) -> stokes_i -> clean
    (gain 1, one iteration) -> restore with beam_from_axes(3, 2, 0.5) on
    weight_cases.oncell(), as test_gpu_clean.py runs it.

    The device's restored plane is the host restore of the downloaded model
    and residual, byte for byte.  At the source's pixel the restored value is
    component * 1 (the centre tap) + residual there: the component is within
    TOLERANCE of the flux and the residual within 3 * TOLERANCE of it (the
    bars of test_gpu_clean.py, derived there), so the sum is within 4 *
    TOLERANCE of the flux."""
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
    psf = idg.psf(G, S, c["image_size"], 0.0, st, t["uvw"], t["wn"],
                  t["weights"], sph, t["md"])
    dirty = idg.invert(ns, G, S, c["image_size"], 0.0, 1, st, t["uvw"],
                       t["wn"], wvis, sph, aterms, t["md"], sum_weights=total)
    residual, model, comps, state = idg.clean(
        idg.stokes_i(dirty), idg.stokes_i(psf), gain=1.0, nr_iterations=1,
        max_components=1)
    beam = idg.beam_from_axes(3, 2, 0.5)
    restored = idg.restore(model, residual, beam=beam)

    got = restored.cpu().numpy()
    want = idg.restore(model.cpu().numpy(), residual.cpu().numpy(), beam=beam)
    rec = comps.cpu().numpy().reshape(-1).view(cc.COMPONENT)[0]
    figures = {
        "component_at": [int(rec["y"]), int(rec["x"])],
        "restored_error_over_flux": float(abs(got[py, px] - flux) / flux),
        "tolerance": TOLERANCE,
    }
    print("restore parity: " + json.dumps(figures))
    assert figures["component_at"] == [py, px]
    assert got.tobytes() == want.tobytes()
    assert figures["restored_error_over_flux"] <= TOLERANCE + 3 * TOLERANCE
