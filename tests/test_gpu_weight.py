"""Imaging weights on the device (kernels/weight_mi355x.hip.cpp)
against their host twins (pinned to the contract by test_weight_host.py):
the density bit for bit at every shape where the kernel takes another path,
(a, b), the imaging weights and weighted visibilities bit for bit, the two
double sums within n 2^-52 relative, and weigh -> psf / invert end to end on
the on-cell case."""
import numpy as np
import pytest

import image_cases as ic
import weight_cases as wc
from conftest import TOLERANCE

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def idg():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import idg_amd
    return idg_amd


def _flagged():
    return wc.flagged(wc.planned())[0]


DENSITY_CASES = {
    "planned_in_tile": lambda: wc.planned(),
    "kernel_size_0": lambda: wc.planned(kernel_size=0),
    "generated_outside_tile": lambda: wc.generated(),
    "one_timestep": lambda: wc.planned(B=4, T=40, Tmax=1),
    "one_channel": lambda: wc.planned(C=1),
    "below_one_wave": lambda: wc.planned(B=4, T=7, C=5),
    "S24": lambda: wc.planned(S=24),
    "S64": lambda: wc.planned(S=64),
    "four_w_layers": lambda: wc.planned(w_step=8.0, W=4),
    "one_cell": lambda: wc.one_cell(),
    "flagged": _flagged,
}
_cache = {}


def _case(name):
    """The case, its device tensors and the host twin's density, made once."""
    import idg_amd
    import torch
    if name not in _cache:
        c = DENSITY_CASES[name]()
        t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda()
             for k in ("uvw", "wn", "weights", "vis")}
        t["md"] = torch.from_numpy(np.ascontiguousarray(
            c["md"]).view(np.int32).reshape(-1, 9)).cuda()
        host = idg_amd.weight_density(c["G"], c["S"], c["image_size"],
                                      c["uvw"], c["wn"], c["weights"], c["md"])
        host.setflags(write=False)
        _cache[name] = (c, t, host)
    return _cache[name]


def _guarded(G):
    """A zeroed [G, G] int64 density between two guard rows."""
    import torch
    buf = torch.full((G + 2, G), GUARD, dtype=torch.int64, device="cuda")
    buf[1:G + 1] = 0
    return buf, buf[1:G + 1]


def _dev_density(idg, c, t, md=None, density=None, stream=None):
    return idg.weight_density(c["G"], c["S"], c["image_size"], t["uvw"],
                              t["wn"], t["weights"],
                              t["md"] if md is None else md, density,
                              stream=stream)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- density ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DENSITY_CASES))
def test_density_is_the_hosts(idg, name):
    c, t, host = _case(name)
    assert host.sum() > 0
    # the path each of these three is for
    inside, live = wc.inside_box(c)
    if name == "planned_in_tile":
        assert inside == live > 0
    if name == "kernel_size_0":
        assert 0 < live - inside < live
    if name == "generated_outside_tile":
        assert inside == 0 < live
    buf, d = _guarded(c["G"])
    assert _dev_density(idg, c, t, density=d) is d
    got = _u64(buf)
    assert np.all(got[0] == np.int64(GUARD).view(np.uint64))
    assert np.all(got[-1] == np.int64(GUARD).view(np.uint64))
    assert np.array_equal(got[1:-1], host)


def test_density_of_no_subgrids(idg):
    import torch
    c, t, host = _case("planned_in_tile")
    d = torch.full((c["G"], c["G"]), 5, dtype=torch.int64, device="cuda")
    _dev_density(idg, c, t, md=t["md"][:0], density=d)
    assert bool((d == 5).all())


def test_density_same_bytes_again_reversed_and_on_a_stream(idg):
    import torch
    c, t, host = _case("planned_in_tile")
    first, second = _dev_density(idg, c, t), _dev_density(idg, c, t)
    assert np.array_equal(_u64(first), host)
    assert np.array_equal(_u64(second), host)
    # (a plan's baseline_offset is 0 in every record, so any order of the
    # records indexes the same rows)
    rev = t["md"].flip(0).contiguous()
    assert np.array_equal(_u64(_dev_density(idg, c, t, md=rev)), host)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    d = _dev_density(idg, c, t, stream=stream)
    stream.synchronize()
    assert np.array_equal(_u64(d), host)
    idg.release_workspaces(stream)


def test_density_accumulates_over_batches(idg):
    c, t, host = _case("planned_in_tile")
    half = c["md"].size // 2
    d = _dev_density(idg, c, t, md=t["md"][:half].contiguous())
    _dev_density(idg, c, t, md=t["md"][half:].contiguous(), density=d)
    assert np.array_equal(_u64(d), host)


# ---- scheme --------------------------------------------------------------------
@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("scheme", wc.SCHEMES)
def test_scheme_is_the_hosts(idg, scheme, hermitian):
    import torch
    c, t, host = _case("planned_in_tile")
    d = torch.from_numpy(host.view(np.int64).copy()).cuda()
    runs = [idg.weight_scheme(c["G"], d, scheme, 0.5, hermitian=hermitian)
            .cpu().numpy() for _ in range(2)]
    want = idg.weight_scheme(c["G"], np.array(host), scheme, 0.5,
                             hermitian=hermitian)
    assert runs[0][0] == want[0]
    assert wc.ulps_apart(runs[0][1], want[1]) <= (scheme == "briggs")
    assert np.array_equal(_bits(runs[0]), _bits(runs[1]))
    if scheme == "briggs":
        assert want[1] > 0


# ---- apply ---------------------------------------------------------------------
def _dev_apply(idg, c, t, d, ab, vis="own", **kw):
    return idg.weight_apply(c["G"], c["image_size"], t["uvw"], t["wn"],
                            t["weights"], t["md"], d, ab,
                            t["vis"] if isinstance(vis, str) else vis, **kw)


@pytest.mark.parametrize("name", ["planned_in_tile", "generated_outside_tile",
                                  "flagged", "below_one_wave"])
@pytest.mark.parametrize("scheme", wc.SCHEMES)
def test_apply_is_the_hosts(idg, name, scheme):
    import torch
    c, t, host = _case(name)
    d = _dev_density(idg, c, t)
    ab = idg.weight_scheme(c["G"], d, scheme, 0.0)
    rows, C = c["weights"].shape
    cov = wc.cover(c["md"], rows) > 0
    iw0 = torch.full((rows, C), -7.0, device="cuda")
    out0 = torch.full((rows, C, 4, 2), -9.0, device="cuda")
    runs = [_dev_apply(idg, c, t, d, ab, imaging_weights=iw0.clone(),
                       out=out0.clone()) for _ in range(2)]
    iw, out, total = (x.cpu().numpy() for x in runs[0])
    # the host twin, fed the device's own (a, b)
    hiw, hout, htotal = idg.weight_apply(
        c["G"], c["image_size"], c["uvw"], c["wn"], c["weights"], c["md"],
        np.array(host), ab.cpu().numpy(), c["vis"],
        imaging_weights=np.full((rows, C), -7.0, F),
        out=np.full((rows, C, 4, 2), -9.0, F))
    assert np.array_equal(_bits(iw), _bits(hiw))
    assert np.array_equal(_bits(out), _bits(hout))
    assert np.all(iw[~cov] == -7.0) and np.all(out[~cov] == -9.0)
    assert hiw[cov].max() > 0
    n = int(cov.sum()) * C
    print(f"sum_weights {name} {scheme}: device {total[0]!r} host "
          f"{htotal[0]!r}")
    assert abs(total[0] - htotal[0]) <= n * 2.0 ** -52 * htotal[0]
    assert total[0] == runs[1][2].cpu().numpy()[0]
    # in place == out of place on the covered rows, untouched elsewhere
    vis = t["vis"].clone()
    iw2, out2, total2 = _dev_apply(idg, c, t, d, ab, vis=vis, out=vis)
    assert out2 is vis
    v = vis.cpu().numpy()
    assert np.array_equal(_bits(v[cov]), _bits(out[cov]))
    assert np.array_equal(_bits(v[~cov]), _bits(c["vis"][~cov]))
    assert total2.cpu().numpy()[0] == total[0]
    # no visibilities: (f, 0, 0, f)
    iw3, out3, _ = _dev_apply(idg, c, t, d, ab, vis=None)
    want = np.zeros((rows, C, 4, 2), F)
    want[:, :, 0, 0] = want[:, :, 3, 0] = np.where(cov[:, None], iw, 0)
    assert np.array_equal(_bits(out3.cpu().numpy()), _bits(want))


def test_apply_of_no_subgrids(idg):
    import torch
    c, t, host = _case("planned_in_tile")
    d = torch.zeros((c["G"], c["G"]), dtype=torch.int64, device="cuda")
    ab = idg.weight_scheme(c["G"], d, "briggs")
    assert ab.cpu().tolist() == [1.0, 0.0]
    iw0 = torch.full(c["weights"].shape, -7.0, device="cuda")
    iw, out, total = idg.weight_apply(
        c["G"], c["image_size"], t["uvw"], t["wn"], t["weights"],
        t["md"][:0], d, ab, None, imaging_weights=iw0,
        sum_weights=torch.ones(1, dtype=torch.float64, device="cuda"))
    assert bool((iw == -7.0).all()) and float(total) == 0.0


# ---- end to end on the on-cell case ----------------------------------------------
def _complex(t):
    a = t.cpu().numpy()
    return a[..., 0].astype(np.float64) + 1j * a[..., 1]


@pytest.fixture(scope="module")
def oncell(idg):
    import torch
    rng = np.random.default_rng(11)
    c = wc.oncell()
    c["weights"] = rng.uniform(0.5, 2.0, c["weights"].shape).astype(F)
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda()
         for k in ("uvw", "wn", "weights", "vis")}
    t["md"] = torch.from_numpy(c["md"].view(np.int32).reshape(-1, 9)).cuda()
    t["spheroidal"] = torch.from_numpy(c["case"]["spheroidal"]).cuda()
    t["aterms"] = torch.from_numpy(c["case"]["aterms"]).cuda()
    return c, t


@pytest.mark.parametrize("scheme", ["natural", "uniform"])
def test_psf_is_the_transform_of_the_weighted_histogram(idg, oncell, scheme):
    c, t = oncell
    G, S, st = c["G"], c["S"], c["case"]["nr_stations"]
    image = idg.psf(G, S, c["image_size"], 0.0, st, t["uvw"], t["wn"],
                    t["weights"], t["spheroidal"], t["md"], scheme=scheme)
    got = _complex(image)
    # the same weights on the host, summed per cell
    d = idg.weight_density(G, S, c["image_size"], c["uvw"], c["wn"],
                           c["weights"], c["md"])
    ab = idg.weight_scheme(G, d, scheme)
    iw, _, total = idg.weight_apply(G, c["image_size"], c["uvw"], c["wn"],
                                    c["weights"], c["md"], d, ab)
    _, X, Y = wc.sample_q(G, c["image_size"], c["uvw"], c["wn"], c["weights"])
    hist = np.zeros((G, G))
    np.add.at(hist, (Y.ravel(), X.ravel()), iw.astype(np.float64).ravel())
    grid = np.zeros((1, 4, G, G), complex)
    grid[0, 0] = grid[0, 3] = hist
    want = ic.grid_to_image(grid, c["image_size"], 0.0) / total[0]
    assert abs(want[0, G // 2, G // 2] - 1) < 1e-12
    centre = got[[0, 3], G // 2, G // 2]
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"psf {scheme}: centre {centre}, max-abs over peak {err:.3e}")
    assert np.abs(centre - 1).max() <= TOLERANCE
    assert err <= TOLERANCE


@pytest.mark.parametrize("scheme", ["natural", "uniform"])
def test_invert_divides_by_the_sum_of_weights(idg, oncell, scheme):
    c, t = oncell
    G, S, st = c["G"], c["S"], c["case"]["nr_stations"]
    ns = c["md"].size
    iw, vis, total, d, ab = idg.weigh(G, S, c["image_size"], t["uvw"],
                                      t["wn"], t["weights"], t["md"],
                                      t["vis"], scheme=scheme)
    args = (ns, G, S, c["image_size"], 0.0, 1, st, t["uvw"], t["wn"], vis,
            t["spheroidal"], t["aterms"], t["md"])
    plain = _complex(idg.invert(*args))
    normed = _complex(idg.invert(*args, sum_weights=total))
    want = plain / float(total)
    err = np.abs(normed - want).max() / np.abs(want).max()
    print(f"invert / sum_weights {scheme}: {err:.3e}")
    assert err <= TOLERANCE
    assert abs(normed[0, G // 2, G // 2] - 1) <= TOLERANCE


def test_invert_without_the_keyword_is_unchanged(idg, oncell):
    import torch
    c, t = oncell
    G, S, st = c["G"], c["S"], c["case"]["nr_stations"]
    ns = c["md"].size
    args = (ns, G, S, c["image_size"], 0.0, 1, st, t["uvw"], t["wn"],
            t["vis"], t["spheroidal"], t["aterms"], t["md"])
    got = idg.invert(*args)
    # what invert did before it knew sum_weights, step by step
    grid = torch.zeros((1, 4, G, G, 2), dtype=torch.float32, device="cuda")
    scaled = torch.full((G, G), 1.0 / float(S * S), dtype=torch.float32,
                        device="cuda")
    idg.grid_onto(*args, grid)
    want = idg.grid_to_image(G, c["image_size"], 0.0, grid, None, 1, scaled)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want.cpu().numpy()))
    assert float(got.abs().max()) > 0
