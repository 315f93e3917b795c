"""Multi-scale CLEAN on the device (kernels/multiscale_mi355x.hip.cpp; DESIGN.md
§17) against its host twins (pinned to the contract by
test_multiscale_host.py): the bytes of every output, guard rows included, of
the convolution, the prepare step and the minor cycle at every case of the
host list; Ns = 1 against the Hogbom host entry; then weigh -> psf / invert ->
clean_multiscale -> predict end to end on the on-cell case."""
import json

import numpy as np
import pytest

import clean_cases as cc
import image_cases as ic
import multiscale_cases as mc
import plan_cases as pc
import weight_cases as wc
from conftest import TOLERANCE

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def idg():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import idg_amd
    return idg_amd


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inner(t, shape):
    return t[1:-1].view(shape)


# ---- convolution -------------------------------------------------------------------
def _conv_device(idg, image, taps, in_place=False, stream=None):
    """(tmp, out) allocations with their guard rows, as numpy."""
    import torch
    G = image.shape[0]
    tmp = _dev(mc.guarded(np.zeros((G, G), F)))
    out = _dev(mc.guarded(image if in_place else np.zeros((G, G), F)))
    src = _inner(out, (G, G)) if in_place else _dev(image)
    torch.cuda.synchronize()
    got = idg.convolve_separable(src, taps, out=_inner(out, (G, G)),
                                 tmp=_inner(tmp, (G, G)), stream=stream)
    assert got.data_ptr() == _inner(out, (G, G)).data_ptr()
    if stream is not None:
        stream.synchronize()
    return tmp.cpu().numpy(), out.cpu().numpy()


_conv_host = {}


def _conv_case(idg, name):
    if name not in _conv_host:
        image, scale = mc.CONV[name]()
        taps, = idg.ms_scale_taps([scale])
        G = image.shape[0]
        tmp, out = (mc.guarded(np.zeros((G, G), F)) for _ in range(2))
        idg.convolve_separable(image, taps, out=mc.inner(out, (G, G)),
                               tmp=mc.inner(tmp, (G, G)))
        _conv_host[name] = (image, taps, tmp, out)
    return _conv_host[name]


@pytest.mark.parametrize("name", sorted(mc.CONV))
def test_convolution_is_the_host(idg, name):
    image, taps, want_tmp, want = _conv_case(idg, name)
    tmp, out = _conv_device(idg, image, taps)
    assert tmp.tobytes() == want_tmp.tobytes()
    assert out.tobytes() == want.tobytes()
    _, again = _conv_device(idg, image, taps, in_place=True)
    assert again.tobytes() == want.tobytes()


def test_convolution_on_a_stream_and_unaligned(idg):
    import torch
    image, taps, want_tmp, want = _conv_case(idg, "G260_r48_vector")
    stream = torch.cuda.Stream()
    tmp, out = _conv_device(idg, image, taps, stream=stream)
    assert out.tobytes() == want.tobytes()
    # G % 4 == 0 but the plane starts 4 bytes off a 16-byte boundary: the
    # scalar instantiation, the same bytes
    G = image.shape[0]
    flat = torch.zeros(G * G + 1, dtype=torch.float32, device="cuda")
    src = flat[1:].view(G, G)
    assert src.data_ptr() % 16 == 4
    src.copy_(_dev(image))
    got = idg.convolve_separable(src, _dev(taps))
    assert got.cpu().numpy().tobytes() == mc.inner(want, (G, G)).tobytes()


def test_convolution_refusals(idg):
    import torch
    image = torch.ones((6, 6), device="cuda")
    other = torch.zeros((6, 6), device="cuda")
    taps = np.ones(3, F)
    for kw in (dict(tmp=image), dict(out=other, tmp=other)):
        with pytest.raises(idg.IdgError) as e:
            idg.convolve_separable(image, taps, **kw)
        assert e.value.code == -1
    with pytest.raises(idg.IdgError):
        idg.convolve_separable(torch.ones((120, 120), device="cuda"),
                               np.ones(99, F))
    torch.cuda.synchronize()
    assert bool((image == 1).all()) and not bool(other.any())


# ---- prepare -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.PREP))
def test_prepare_is_the_host(idg, name):
    import torch
    c = mc.PREP[name]()
    residual, psf, taps = mc.prep_inputs(c, idg)
    Ns, G, Gp = len(taps), c["G"], c["Gp"]
    pairs = Ns * (Ns + 1) // 2
    want_planes, want_cross = idg.ms_prepare(residual, psf, taps)
    planes = _dev(mc.guarded(np.zeros((Ns, G, G), F)))
    cross = _dev(mc.guarded(np.zeros((pairs, Gp, Gp), F)))
    tmp = _dev(mc.guarded(np.zeros((G, G), F)))
    torch.cuda.synchronize()
    idg.ms_prepare(_dev(residual), _dev(psf), taps,
                   planes=_inner(planes, (Ns, G, G)),
                   cross_psf=_inner(cross, (pairs, Gp, Gp)),
                   tmp=_inner(tmp, (G, G)))
    planes, cross, tmp = (t.cpu().numpy() for t in (planes, cross, tmp))
    assert planes[1:-1].tobytes() == want_planes.tobytes()
    assert cross[1:-1].tobytes() == want_cross.tobytes()
    assert planes[1:1 + G].tobytes() == residual.tobytes()
    assert cross[1:1 + Gp].tobytes() == psf.tobytes()
    assert mc.guards_ok(planes) and mc.guards_ok(cross) and mc.guards_ok(tmp)


# ---- the minor cycle -----------------------------------------------------------------
_cache = {}


def _case(idg, name):
    """The case, its inputs and the buffers the host entry leaves, made once."""
    if name not in _cache:
        c = mc.MS[name]()
        i = mc.ms_inputs(c, idg)
        host = mc.run_host(idg, c, i)
        for a in host.values():
            a.setflags(write=False)
        _cache[name] = (c, i, host)
    return _cache[name]


def _upload(b):
    return dict(planes=_dev(b["planes"]), model=_dev(b["model"]),
                components=_dev(b["components"].view(np.int32).reshape(-1, 4)),
                state=_dev(b["state"].view(np.int32).reshape(7)))


def _download(t):
    return dict(planes=t["planes"].cpu().numpy(),
                model=t["model"].cpu().numpy(),
                components=t["components"].cpu().numpy().reshape(-1).view(
                    mc.COMPONENT),
                state=t["state"].cpu().numpy().view(mc.STATE))


def _run_device(idg, c, i, stream=None, check_every=None):
    import torch
    Ns, G = len(c["scales"]), c["G"]
    t = _upload(mc.ms_buffers(c, i))
    cross = _dev(i["cross"])
    mask = None if c["mask"] is None else _dev(c["mask"])
    torch.cuda.synchronize()
    for n in c["chunks"]:
        out = idg.ms_clean(_inner(t["planes"], (Ns, G, G)), cross, i["taps"],
                           i["weight"], i["inv_peak"],
                           model=_inner(t["model"], (G, G)), mask=mask,
                           nr_iterations=n, components=t["components"][1:-1],
                           state=t["state"], check_every=check_every,
                           stream=stream, **mc.ms_params(c))
    assert out[0].data_ptr() == t["planes"][1:-1].data_ptr()
    if stream is not None:
        stream.synchronize()
    return _download(t)


@pytest.mark.parametrize("name", sorted(mc.MS))
def test_minor_cycle_is_the_host(idg, name):
    c, i, host = _case(idg, name)
    got = _run_device(idg, c, i)
    st = got["state"][0]
    print(f"{name}: n_components {st['n_components']} reason {st['reason']} "
          f"peak {st['peak']!r} at {st['peak_index']} scale {st['peak_scale']}")
    assert mc.same_bytes(got, host) == []
    assert mc.ms_guards_ok(got)


@pytest.mark.parametrize("name", ["G260_Gp65_footprint_across_tiles",
                                  "chunks_3_4_5", "mask_hides_the_maximum"])
def test_same_bytes_on_a_stream(idg, name):
    import torch
    c, i, host = _case(idg, name)
    stream = torch.cuda.Stream()
    assert mc.same_bytes(_run_device(idg, c, i, stream=stream), host) == []
    idg.release_workspaces(stream)


@pytest.mark.parametrize("name", ["G260_Gp65_footprint_across_tiles",
                                  "G66_Gp33_scalar_form"])
def test_same_bytes_with_every_tile_rescanning(idg, name, monkeypatch):
    c, i, host = _case(idg, name)
    monkeypatch.setenv("IDG_CLEAN_RESCAN", "1")
    assert mc.same_bytes(_run_device(idg, c, i), host) == []


@pytest.mark.parametrize("name", ["G260_Gp65_footprint_across_tiles",
                                  "stop_below_level", "stop_components_full",
                                  "chunks_3_4_5"])
def test_check_every_4_is_check_every_none(idg, name):
    c, i, host = _case(idg, name)
    assert mc.same_bytes(_run_device(idg, c, i, check_every=4), host) == []


def test_refusals_leave_the_buffers(idg):
    import torch
    c, i, _ = _case(idg, "still_running")
    Ns, G = len(c["scales"]), c["G"]
    before = mc.ms_buffers(c, i)
    t = _upload(before)
    cross = _dev(i["cross"])
    args = (_inner(t["planes"], (Ns, G, G)), cross, i["taps"])
    kw = dict(model=_inner(t["model"], (G, G)),
              components=t["components"][1:-1], state=t["state"],
              **mc.ms_params(c))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(gain=nan), dict(threshold=-1.0),
                dict(cycle_fraction=inf), dict(nr_iterations=-1),
                dict(max_components=-1)):
        with pytest.raises(idg.IdgError) as e:
            idg.ms_clean(*args, i["weight"], i["inv_peak"], **dict(kw, **bad))
        assert e.value.code == -1
    for w, p in (([1, nan, 1], i["inv_peak"]), (i["weight"], [1, 1, inf])):
        with pytest.raises(idg.IdgError) as e:
            idg.ms_clean(*args, w, p, **kw)
        assert e.value.code == -1
    with pytest.raises(idg.IdgError):          # radius 49
        idg.ms_clean(args[0], cross, i["taps"][:2] + [np.ones(99, F)],
                     i["weight"], i["inv_peak"], **kw)
    torch.cuda.synchronize()
    assert mc.same_bytes(_download(t), before) == []
    # a state the device cannot refuse: no iteration runs on it
    t["state"][0] = 6
    idg.ms_clean(*args, i["weight"], i["inv_peak"], **kw)
    got = _download(t)
    assert got["state"][0]["n_components"] == 6 and got["state"][0]["peak"] > 0
    for k in ("planes", "model", "components"):
        assert got[k].tobytes() == before[k].tobytes()


# ---- clean_multiscale: Ns = 1 is Hogbom; carried planes ----------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_one_scale_is_hogbom(idg, name):
    import torch
    c = cc.CASES[name]()
    want = cc.run_host(idg, c)
    b = cc.buffers(c)
    M = max(c["max_components"], 1)
    residual, model = _dev(b["residual"]), _dev(b["model"])
    comps = torch.zeros((M, 4), dtype=torch.int32, device="cuda")
    state = torch.zeros(7, dtype=torch.int32, device="cuda")
    mask = None if c["mask"] is None else _dev(c["mask"])
    planes = cross = None
    for n in c["chunks"]:
        out = idg.clean_multiscale(
            residual[1:-1], _dev(c["psf"]), scales=(0,), model=model[1:-1],
            mask=mask, nr_iterations=n, components=comps, state=state,
            planes=planes, cross_psf=cross, **cc.params(c))
        planes, cross = out[4:]
    assert out[0].data_ptr() == residual[1:-1].data_ptr()
    assert residual.cpu().numpy().tobytes() == want["residual"].tobytes()
    assert model.cpu().numpy().tobytes() == want["model"].tobytes()
    comps = comps.cpu().numpy().reshape(-1).view(mc.COMPONENT)
    state = state.cpu().numpy().view(mc.STATE)
    old = want["components"][1:-1]
    for k in ("y", "x", "value"):
        assert comps[k].tobytes() == old[k].tobytes()
    assert not comps["scale"].any()
    for k in cc.STATE.names:
        assert state[k].tobytes() == want["state"][k].tobytes(), k
    assert state[0]["peak_scale"] == (0 if state[0]["peak_index"] >= 0 else -1)


def test_clean_multiscale_chunked_on_a_stream_is_the_host(idg):
    """Prepare and 3 + 4 + 5 iterations with planes and cross_psf carried
    across the calls, on a second stream with check_every=4, against one host
    call of 12."""
    import torch
    dirty, psf = mc.property_field()
    kw = dict(scales=(0, 4, 8, 16), gain=0.1, threshold=0.3,
              max_components=12)
    want = idg.clean_multiscale(dirty.copy(), psf, **kw)
    stream = torch.cuda.Stream()
    residual, dpsf = _dev(dirty), _dev(psf)
    torch.cuda.synchronize()
    model = comps = state = planes = cross = None
    for n in (3, 4, 5):
        residual, model, comps, state, planes, cross = idg.clean_multiscale(
            residual, dpsf, model=model, components=comps, state=state,
            planes=planes, cross_psf=cross, nr_iterations=n, check_every=4,
            stream=stream, **kw)
    stream.synchronize()
    got = (residual, model, comps, state, planes, cross)
    assert want[3][0]["n_components"] == 12
    for g, w in zip(got, want):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    idg.release_workspaces(stream)


# ---- end to end on the on-cell case ----------------------------------------------
def _pairs(z):
    return _dev(np.stack([z.real, z.imag], axis=-1).astype(F))


def test_a_point_source_through_the_chain(idg):
    """test_gpu_clean.py's end-to-end test with clean_multiscale in clean's
    place, to the same bars (taken from that file): weigh (natural) -> psf ->
    invert(sum_weights=) -> stokes_i -> clean_multiscale (gain 1, one
    iteration, Gp = G) -> predict on weight_cases.oncell().  The source is a
    point, so the component must be of scale 0, where it is Hogbom's.

    Scales (0, 4): the on-cell array has no baseline shorter than 14 uv cells,
    so its PSF holds nothing as smooth as the larger default scales: 1 /
    cross(s, s)[centre] is 3.2 at scale 4, 35 at scale 8 and 3 * 10^4 at scale
    16, where the search then amplifies the truncated PSF's edge instead of
    the source ("Scales the PSF does not support")."""
    import torch
    c = wc.oncell()
    G, S, st = c["G"], c["S"], c["case"]["nr_stations"]
    flux, py, px = 2.5, G // 2 + 3, G // 2 - 5
    host = dict(c["case"], geom=dict(pc.ONCELL, C=1), md=c["md"], W=1,
                w_step=0.0)
    sky = np.zeros((4, G, G), complex)
    sky[0, py, px] = sky[3, py, px] = flux
    vis_in = ic.direct_predict(host, sky)
    t = {k: _dev(c[k]) for k in ("uvw", "wn", "weights")}
    t["vis"] = _pairs(vis_in)
    t["md"] = _dev(c["md"].view(np.int32).reshape(-1, 9))
    sph = _dev(c["case"]["spheroidal"])
    aterms = _dev(c["case"]["aterms"])
    ns = c["md"].size

    iw, wvis, total, density, ab = idg.weigh(
        G, S, c["image_size"], t["uvw"], t["wn"], t["weights"], t["md"],
        t["vis"])
    beam = idg.psf(G, S, c["image_size"], 0.0, st, t["uvw"], t["wn"],
                   t["weights"], sph, t["md"])
    dirty = idg.invert(ns, G, S, c["image_size"], 0.0, 1, st, t["uvw"],
                       t["wn"], wvis, sph, aterms, t["md"], sum_weights=total)
    residual, model, comps, state, planes, cross = idg.clean_multiscale(
        idg.stokes_i(dirty).contiguous(), idg.stokes_i(beam).contiguous(),
        scales=(0, 4), gain=1.0, nr_iterations=1, max_components=1)
    rec = comps.cpu().numpy().reshape(-1).view(mc.COMPONENT)[0]
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
        "component_at": [int(rec["y"]), int(rec["x"]), int(rec["scale"])],
        "component_error_over_flux": float(abs(rec["value"] - flux) / flux),
        "residual_max_over_flux": float(np.abs(patch).max() / flux),
        "predict_max_abs_over_flux": float(
            np.abs(out[rows] - vis_in[rows]).max() / flux),
        "tolerance": TOLERANCE,
    }
    print("multiscale parity: " + json.dumps(figures))
    assert figures["component_at"] == [py, px, 0]
    assert int(state.cpu()[0]) == 1 and rows.sum() > 0
    assert figures["component_error_over_flux"] <= TOLERANCE
    assert figures["residual_max_over_flux"] <= 3 * TOLERANCE
    assert figures["predict_max_abs_over_flux"] <= 3 * TOLERANCE
