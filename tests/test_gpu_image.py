"""Grid <-> image on the device (kernels/image_mi355x.hip.cpp):
grid_fft_launch against numpy's float64 transform, grid_to_image /
image_to_grid against their float64 restatement (tests/image_cases.py), and
plan_launch -> invert / predict against the oracle chain of
test_image_host.py.  Every bar is a yardstick computed here: a complex64
transform or restatement of the same input."""
import numpy as np
import pytest

import image_cases as ic
import pipeline_oracle as pl
import plan_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def idg():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import idg_amd
    return idg_amd


def _pairs(c):
    import torch
    return torch.from_numpy(pl.to_pairs(c)).cuda()


def _complex(t):
    a = t.cpu().numpy()
    return a[..., 0].astype(np.float64) + 1j * a[..., 1]


# ---- grid_fft_launch --------------------------------------------------------
def _fft_case(G, planes, seed):
    """float32 input, its float64 transforms by numpy, and the bar: 4 x the
    error of torch's complex64 transform on the CPU."""
    import torch
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(planes, G, G)) + 1j * rng.normal(
        size=(planes, G, G))).astype(np.complex64)
    ref = {-1: np.fft.fft2(x.astype(np.complex128)),
           +1: np.fft.ifft2(x.astype(np.complex128)) * (G * G)}
    single = torch.fft.fft2(torch.from_numpy(x)).numpy()
    bar = 4 * ic.rel_max(single, ref[-1])
    return x, ref, bar


FFT_CASES = [(64, 1, +1, 1.0), (64, 8, -1, 0.37), (128, 1, -1, 1.0),
             (128, 8, +1, 0.37), (1024, 1, +1, 0.37), (1024, 8, -1, 1.0),
             (2048, 1, -1, 0.37), (2048, 8, +1, 1.0), (4096, 1, -1, 1.0)]


@pytest.mark.parametrize("G,planes,sign,scale", FFT_CASES)
def test_grid_fft_against_float64(idg, G, planes, sign, scale):
    x, ref, bar = _fft_case(G, planes, G + planes)
    t = _pairs(x)
    idg.grid_fft_launch(t, sign, scale)
    err = ic.rel_max(_complex(t), ref[sign] * np.float32(scale))
    print(f"G = {G}, {planes} planes, sign {sign:+d}: {err:.3e} (bar "
          f"{bar:.3e})")
    assert err <= bar


@pytest.mark.parametrize("G", [64, 128, 1024])
def test_grid_fft_there_and_back(idg, G):
    x, _, bar = _fft_case(G, 2, G)
    t = _pairs(x)
    idg.grid_fft_launch(t, +1)
    idg.grid_fft_launch(t, -1, 1.0 / (G * G))
    err = ic.rel_max(_complex(t), x.astype(np.complex128))
    print(f"G = {G} there and back: {err:.3e} (bar {bar:.3e})")
    assert err <= bar


@pytest.mark.parametrize("G,y0,x0,sign", [(64, 3, 5, +1), (128, 77, 1, -1),
                                          (1024, 513, 300, +1)])
def test_grid_fft_of_a_delta_is_the_plane_wave(idg, G, y0, x0, sign):
    import torch
    t = torch.zeros((1, G, G, 2), dtype=torch.float32, device="cuda")
    t[0, y0, x0, 0] = 1.0
    idg.grid_fft_launch(t, sign)
    got = _complex(t)[0]
    k = np.arange(G)
    want = np.exp(sign * 2j * np.pi * ((k[:, None] * y0 + k[None, :] * x0)
                                       % G) / G)
    assert np.abs(got - want).max() < 1e-6
    for part in (np.real, np.imag):
        sure = np.abs(part(want)) > 1e-3
        assert np.array_equal(np.sign(part(got))[sure],
                              np.sign(part(want))[sure])


def test_grid_fft_rejects_other_sizes(idg):
    import ctypes
    import torch
    from idg_amd._lib import lib
    for G in (96, 8192, 32):
        with pytest.raises(ValueError):
            # (refused on its shape, before the buffer is looked at)
            idg.grid_fft_launch(torch.empty((1, G, G, 2), device="meta"), 1)
        # the C entry refuses before it touches the buffer
        assert lib.idg_grid_fft_launch(G, 1, 1, ctypes.c_float(1.0), None,
                                       None) == -1
        assert str(G).encode() in lib.idg_last_error()
        assert lib.idg_grid_to_image_launch(
            G, 1, ctypes.c_float(0.1), ctypes.c_float(0.0), None, None, None,
            None) == -1
    t = torch.zeros((1, 64, 64, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        idg.grid_fft_launch(t, 0)


# ---- grid_to_image / image_to_grid ------------------------------------------
# (both exact in float32, which is what the entries take)
IMAGE_SIZE, W_STEP = 0.203125, 4000.0   # layer 0 at the corner: 130 rad
# (from G = 2048 the image-side work is a launch of its own: another path)
STEP_CASES = [(128, 1, True), (128, 3, False), (1024, 1, False),
              (1024, 3, True), (2048, 2, True)]


def _step_inputs(G, W, with_correction):
    rng = np.random.default_rng(G + W)
    cplx = lambda *s: (rng.normal(size=s) + 1j * rng.normal(size=s)).astype(
        np.complex64)
    corr = rng.uniform(0.5, 2.0, (G, G)).astype(np.float32) \
        if with_correction else None
    n_corner = ic.n_of(ic.lm(G, IMAGE_SIZE), ic.lm(G, IMAGE_SIZE))[0, 0]
    assert 2 * np.pi * W_STEP * 0.5 * n_corner > 100.0
    return cplx(W, 4, G, G), cplx(4, G, G), corr


@pytest.mark.parametrize("G,W,with_correction", STEP_CASES)
def test_grid_to_image_against_the_restatement(idg, G, W, with_correction):
    import torch
    grid, _, corr = _step_inputs(G, W, with_correction)
    want = ic.grid_to_image(grid, IMAGE_SIZE, W_STEP, corr)
    bar = 4 * ic.rel_max(ic.grid_to_image(grid, IMAGE_SIZE, W_STEP, corr,
                                          single=True), want)
    got = idg.grid_to_image(
        G, IMAGE_SIZE, W_STEP, _pairs(grid), nr_w_layers=W,
        correction=None if corr is None else torch.from_numpy(corr).cuda())
    err = ic.rel_max(_complex(got), want)
    print(f"grid_to_image G = {G}, W = {W}: {err:.3e} (bar {bar:.3e})")
    assert err <= bar


@pytest.mark.parametrize("G,W,with_correction", STEP_CASES)
def test_image_to_grid_against_the_restatement(idg, G, W, with_correction):
    import torch
    _, image, corr = _step_inputs(G, W, with_correction)
    want = ic.image_to_grid(image, W, IMAGE_SIZE, W_STEP, corr)
    bar = 4 * ic.rel_max(ic.image_to_grid(image, W, IMAGE_SIZE, W_STEP, corr,
                                          single=True), want)
    grid = torch.full((W, 4, G, G, 2), 7.0, dtype=torch.float32,
                      device="cuda")          # every layer is overwritten
    idg.image_to_grid(
        G, IMAGE_SIZE, W_STEP, _pairs(image), grid, nr_w_layers=W,
        correction=None if corr is None else torch.from_numpy(corr).cuda())
    err = ic.rel_max(_complex(grid), want)
    print(f"image_to_grid G = {G}, W = {W}: {err:.3e} (bar {bar:.3e})")
    assert err <= bar


@pytest.mark.parametrize("G,W", [(128, 3), (1024, 1)])
def test_the_two_steps_are_adjoint(idg, G, W):
    import torch
    grid, image, corr = _step_inputs(G, W, True)
    want = ic.grid_to_image(grid, IMAGE_SIZE, W_STEP, corr)
    bar = 4 * ic.rel_max(ic.grid_to_image(grid, IMAGE_SIZE, W_STEP, corr,
                                          single=True), want)
    c = torch.from_numpy(corr).cuda()
    up = _complex(idg.image_to_grid(G, IMAGE_SIZE, W_STEP, _pairs(image),
                                    nr_w_layers=W, correction=c))
    down = _complex(idg.grid_to_image(G, IMAGE_SIZE, W_STEP, _pairs(grid),
                                      nr_w_layers=W, correction=c))
    a = np.vdot(up, grid.astype(np.complex128))
    b = np.vdot(image.astype(np.complex128), down)
    print(f"adjointness G = {G}, W = {W}: {abs(a - b) / abs(a):.3e} (bar "
          f"{bar:.3e})")
    assert abs(a - b) <= bar * abs(a)


@pytest.mark.parametrize("G", [128, 1024])
def test_one_layer_without_w_is_the_shifted_grid_fft(idg, G):
    grid, _, _ = _step_inputs(G, 1, False)
    _, _, bar = _fft_case(G, 1, G)
    flip = ic.centre_flip(G)
    t = _pairs(grid[0] * flip)
    idg.grid_fft_launch(t, -1)
    want = _complex(t) * flip
    got = _complex(idg.grid_to_image(G, IMAGE_SIZE, 0.0, _pairs(grid)))
    assert ic.rel_max(got, want) <= bar


# ---- end to end -------------------------------------------------------------
def _device_case(idg, case):
    """plan_launch on the case's tracks; the case with the device's metadata
    and the tensors the launches take."""
    import torch
    o = case.get("geom", ic.SMALL)
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in
         ("uvw", "baselines", "wn", "vis", "aterms", "spheroidal")}
    md, counts = idg.plan_launch(o["G"], o["S"], o["image_size"],
                                 case["w_step"], t["uvw"], t["baselines"],
                                 t["wn"], o["K"], o["Tmax"], 0, case["W"])
    ns, dropped = (int(v) for v in counts.cpu())
    assert dropped == 0
    md = md[:ns].contiguous()
    host = dict(case)
    host["md"] = md.cpu().numpy().view(idg.METADATA_DTYPE).reshape(-1)
    return host, t, md, ns


def _oncell():
    o = dict(pc.ONCELL, C=1)
    case = pc.oncell_case()
    case.update(geom=o, W=1, w_step=0.0)
    return case, np.ones((o["G"], o["G"]))


def _multi_channel():
    case = ic.small_case(3, 60.0)
    corr, _ = ic.correction_for(case)
    return case, corr


E2E = {"oncell": _oncell, "multi_channel_W3": _multi_channel}


@pytest.mark.parametrize("which", sorted(E2E))
def test_invert_under_the_device_plan(idg, oracle_lib, which):
    import torch
    case, corr = E2E[which]()
    host, t, md, ns = _device_case(idg, case)
    o = host.get("geom", ic.SMALL)
    image = idg.invert(
        ns, o["G"], o["S"], o["image_size"], host["w_step"], o["C"],
        host["nr_stations"], t["uvw"], t["wn"], t["vis"], t["spheroidal"],
        t["aterms"], md, nr_w_layers=host["W"],
        correction=torch.from_numpy(corr.astype(np.float32)).cuda())
    want = ic.chain_invert(oracle_lib, host, host["vis"],
                           corr.astype(np.float32).astype(np.float64))
    rel = ic.rel_max(_complex(image), want)
    print(f"invert {which} vs the oracle chain: {rel:.3e}")
    assert tuple(image.shape) == (4, o["G"], o["G"], 2)
    assert rel < 1e-5


@pytest.mark.parametrize("which", sorted(E2E))
def test_predict_under_the_device_plan(idg, oracle_lib, which):
    import torch
    case, corr = E2E[which]()
    host, t, md, ns = _device_case(idg, case)
    o = host.get("geom", ic.SMALL)
    G = o["G"]
    rng = np.random.default_rng(4)
    model = np.zeros((4, G, G), np.complex64)
    for y, x in rng.integers(G // 4, 3 * G // 4, (6, 2)):
        model[:, y, x] = rng.normal(size=4) + 1j * rng.normal(size=4)
    vis = torch.zeros_like(t["vis"])
    idg.predict(ns, G, o["S"], o["image_size"], host["w_step"], o["C"],
                host["nr_stations"], t["uvw"], t["wn"], vis, t["spheroidal"],
                t["aterms"], md, _pairs(model), nr_w_layers=host["W"],
                correction=torch.from_numpy(corr.astype(np.float32)).cuda())
    want = ic.chain_predict(oracle_lib, host, model.astype(np.complex128),
                            corr.astype(np.float32).astype(np.float64))
    rel = ic.rel_max(_complex(vis), want)
    print(f"predict {which} vs the oracle chain: {rel:.3e}")
    assert rel < 1e-5


def test_a_point_source_inverts_to_its_pixel(idg):
    import torch
    case, corr = _multi_channel()
    host, t, md, ns = _device_case(idg, case)
    o = ic.SMALL
    model = np.zeros((4, o["G"], o["G"]), complex)
    model[0, 45, 77] = 1.0
    vis = _pairs(ic.direct_predict(host, model))
    image = idg.invert(
        ns, o["G"], o["S"], o["image_size"], host["w_step"], o["C"],
        host["nr_stations"], t["uvw"], t["wn"], vis, t["spheroidal"],
        torch.from_numpy(ic.identity_aterms(host)).cuda(), md,
        nr_w_layers=host["W"],
        correction=torch.from_numpy(corr.astype(np.float32)).cuda())
    got = np.abs(_complex(image)[0])
    assert np.unravel_index(np.argmax(got), got.shape) == (45, 77)
    # every covered visibility adds 1 there
    assert abs(got[45, 77] / (ic.covered_rows(host).sum() * o["C"]) - 1) < 1e-2


# ---- streams, workspaces, extents -------------------------------------------
def test_two_sizes_alternating_on_one_stream(idg):
    import torch
    stream = torch.cuda.Stream()
    inputs = {G: _step_inputs(G, 2, False) for G in (64, 256)}
    want = {G: ic.grid_to_image(v[0], IMAGE_SIZE, 0.0) for G, v in
            inputs.items()}
    bar = {G: 4 * ic.rel_max(ic.grid_to_image(v[0], IMAGE_SIZE, 0.0,
                                              single=True), want[G])
           for G, v in inputs.items()}
    with torch.cuda.stream(stream):
        for G in (64, 256, 64, 256):
            grid = _pairs(inputs[G][0])
            image = idg.grid_to_image(G, IMAGE_SIZE, 0.0, grid, nr_w_layers=2,
                                      stream=stream)
            back = idg.image_to_grid(G, IMAGE_SIZE, 0.0, image, grid,
                                     nr_w_layers=2, stream=stream)
            stream.synchronize()
            assert back is grid
            assert ic.rel_max(_complex(image), want[G]) <= bar[G]
            # and the way back, from the image the device made
            src = _complex(image)
            up = ic.image_to_grid(src, 2, IMAGE_SIZE, 0.0)
            up_bar = 4 * ic.rel_max(ic.image_to_grid(src, 2, IMAGE_SIZE, 0.0,
                                                     single=True), up)
            assert ic.rel_max(_complex(back), up) <= up_bar
    idg.release_workspaces(stream)


def test_invert_and_predict_on_a_stream_of_their_own(idg):
    """stream= given while another stream is current: everything the two
    make themselves (the zeroed grid, the scaled correction, the scratch) must
    be ordered on that stream.  Same bits as on the current stream."""
    import torch
    case, corr = _multi_channel()
    host, t, md, ns = _device_case(idg, case)
    o = ic.SMALL
    c = torch.from_numpy(corr.astype(np.float32)).cuda()
    model = torch.randn((4, o["G"], o["G"], 2), device="cuda",
                        generator=torch.Generator("cuda").manual_seed(1))

    def both(stream):
        image = idg.invert(
            ns, o["G"], o["S"], o["image_size"], host["w_step"], o["C"],
            host["nr_stations"], t["uvw"], t["wn"], t["vis"], t["spheroidal"],
            t["aterms"], md, nr_w_layers=host["W"], correction=c,
            stream=stream)
        vis = torch.zeros_like(t["vis"])
        torch.cuda.synchronize()        # vis is zeroed on the current stream
        idg.predict(ns, o["G"], o["S"], o["image_size"], host["w_step"],
                    o["C"], host["nr_stations"], t["uvw"], t["wn"], vis,
                    t["spheroidal"], t["aterms"], md, model,
                    nr_w_layers=host["W"], correction=c, stream=stream)
        (stream or torch.cuda.current_stream()).synchronize()
        return image.cpu().numpy(), vis.cpu().numpy()

    torch.cuda.synchronize()
    want = both(None)
    stream = torch.cuda.Stream()
    for _ in range(3):
        got = both(stream)
        assert got[0].tobytes() == want[0].tobytes()
        assert got[1].tobytes() == want[1].tobytes()
    idg.release_workspaces(stream)


def test_extent_checks(idg):
    import torch
    G = 64
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        idg.grid_to_image(G, 0.1, 0.0, z(2, 4, G, G, 2), nr_w_layers=3)
    with pytest.raises(ValueError):
        idg.grid_to_image(G, 0.1, 0.0, z(1, 4, G, G, 2), z(4, G, G))
    with pytest.raises(ValueError):
        idg.image_to_grid(G, 0.1, 0.0, z(4, G, G, 2), z(1, 4, G, G, 2),
                          correction=z(G, G - 1))
    with pytest.raises(ValueError):
        idg.image_to_grid(96, 0.1, 0.0, z(4, 96, 96, 2))
    with pytest.raises(ValueError):
        idg.grid_to_image(G, 0.1, 0.0, z(1, 4, G, G, 2), nr_w_layers=0)
    with pytest.raises(ValueError):
        idg.grid_to_image(G, 0.1, 0.0, z(1, 4, G, G, 2), nr_w_layers=16384)
    with pytest.raises(ValueError):
        idg.grid_fft_launch(z(4, G, G), 1)
