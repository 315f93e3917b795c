"""The plan step on the device (idg_plan_launch, kernels/plan_mi355x.hip.cpp;
DESIGN.md §12): bit for bit the host entry idg_plan -- records [0, counts[0])
and both counts -- at every shape at which the wave-per-baseline walk takes
another path, and end to end through the device gridder and adder."""
import numpy as np
import pytest

import pipeline_oracle as pl
import plan_cases as pc
from conftest import TOLERANCE

pytestmark = pytest.mark.gpu
G, S, K, C = 512, 32, 8, 8
SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def idg():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import idg_amd
    return idg_amd


def _device_plan(idg, uvw, bl, wn, w_step=0.0, W=1, A=0, tmax=128,
                 capacity=None, stream=None):
    """plan_launch into a sentinel-filled buffer; numpy (words, counts)."""
    import torch
    B, T = uvw.shape[:2]
    cap = B * T if capacity is None else capacity
    md = torch.full((cap + 2, 9), SENTINEL, dtype=torch.int32, device="cuda")
    out, counts = idg.plan_launch(
        G, S, pc.IMAGE_SIZE, w_step, torch.from_numpy(uvw).cuda(),
        torch.from_numpy(bl).cuda(), torch.from_numpy(wn).cuda(), K, tmax, A,
        W, metadata=md, capacity=cap, stream=stream)
    assert out is md
    if stream is not None:
        stream.synchronize()
    return md.cpu().numpy(), counts.cpu().numpy()


def _agree(idg, uvw, bl, wn, w_step=0.0, W=1, A=0, tmax=128, **kw):
    """Device plan == host plan, bit for bit; nothing written past the need.
    Returns the host plan."""
    ref, dropped = idg.plan(G, S, pc.IMAGE_SIZE, w_step, uvw, bl, wn, K, tmax,
                            A, W)
    words, counts = _device_plan(idg, uvw, bl, wn, w_step, W, A, tmax, **kw)
    assert tuple(counts) == (ref.size, dropped)
    assert np.array_equal(words[:ref.size], ref.view(np.int32).reshape(-1, 9))
    assert np.all(words[ref.size:] == SENTINEL)
    return ref, dropped


@pytest.fixture(scope="module")
def tracks():
    return pc.arc_tracks(12, 300, G, C)


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_host_inputs_and_variants(idg, tracks, variant):
    """T = 300: four full 64-lane blocks and one of 44."""
    w_step, W, A, tmax = variant
    ref, dropped = _agree(idg, *tracks, w_step, W, A, tmax)
    assert dropped == 4 and ref.size >= 24


@pytest.mark.parametrize("T", [1, 5, 64, 65])
@pytest.mark.parametrize("tmax", [1, 48, 64, 128])
def test_short_tracks_and_block_edges(idg, T, tmax):
    """tmax = 128 carries the box across a 64-lane block (baseline 0 is slow
    enough to fill it); T = 65 leaves a one-lane tail block."""
    uvw, bl, wn = pc.arc_tracks(5, 300, G, C, seed=2, bad_rows=False)
    uvw = np.ascontiguousarray(uvw[:, 100:100 + T])
    ref, dropped = _agree(idg, uvw, bl, wn, tmax=tmax)
    assert dropped == 0
    if T >= 64:
        assert ref["nr_timesteps"].max() == min(T, tmax)


@pytest.mark.parametrize("where", ["start", "end"])
def test_a_run_of_invalid_rows_longer_than_a_block(idg, where):
    uvw, bl, wn = pc.arc_tracks(3, 150, G, C, seed=6, bad_rows=False)
    if where == "start":
        uvw[1, :70, 0] = np.nan
    else:
        uvw[1, -70:, 1] = np.inf
    ref, dropped = _agree(idg, uvw, bl, wn)
    assert dropped == 70
    mine = ref[ref["time_offset"] // 150 == 1]
    assert mine["nr_timesteps"].sum() == 80
    assert mine["time_offset"][0] == 150 + (70 if where == "start" else 0)


def test_aterm_slots_that_do_not_divide_a_block(idg):
    uvw, bl, wn = pc.arc_tracks(4, 300, G, C, seed=7, bad_rows=False)
    ref, _ = _agree(idg, uvw, bl, wn, A=50)
    assert set(ref["aterm_index"]) == set(range(6))


def test_one_baseline(idg):
    uvw, bl, wn = pc.arc_tracks(1, 200, G, C, seed=8, bad_rows=False)
    _agree(idg, uvw, bl, wn, w_step=8.0, W=4)


def test_many_short_baselines_cross_the_scan_chunk(idg):
    """B = 2,500 > the scan's 1,024-baseline chunk; T = 3: most waves finish
    in one step."""
    uvw, bl, wn = pc.arc_tracks(12, 300, G, C, seed=9, bad_rows=False)
    B = 2500
    pick = np.random.default_rng(0).integers(0, 12 * 100, B)
    uvw = np.ascontiguousarray(uvw.reshape(-1, 3, 3)[pick])
    uvw[5, 1, 0] = np.nan
    uvw[1030, :, 1] = np.nan                       # empty, past the chunk
    bl = np.stack([np.arange(B) % 60, 60 + np.arange(B) % 7], 1).astype(
        np.int32)
    ref, dropped = _agree(idg, uvw, bl, wn)
    assert dropped == 4 and ref.size >= B


def test_baseline_0_yields_no_subgrid(idg):
    uvw, bl, wn = pc.arc_tracks(3, 40, G, C, seed=3, bad_rows=False)
    uvw[0, :, 0] = np.resize(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38,
                                       1e12, -1e12, 2.0e11], np.float32), 40)
    ref, dropped = _agree(idg, uvw, bl, wn, w_step=8.0, W=4)
    assert dropped == 40
    assert ref["time_offset"][0] == 40 and ref["station1"][0] == bl[1][0]


def test_capacity_below_the_need(idg, tracks):
    uvw, bl, wn = tracks
    ref, dropped = idg.plan(G, S, pc.IMAGE_SIZE, 0.0, uvw, bl, wn, K)
    cap = ref.size // 2
    words, counts = _device_plan(idg, uvw, bl, wn, capacity=cap)
    assert tuple(counts) == (ref.size, dropped)
    assert np.array_equal(words[:cap], ref.view(np.int32).reshape(-1, 9)[:cap])
    assert np.all(words[cap:] == SENTINEL)
    _, counts = _device_plan(idg, uvw, bl, wn, capacity=0)   # counts only
    assert tuple(counts) == (ref.size, dropped)


def test_stream_and_workspace_reuse(idg, tracks):
    import torch
    stream = torch.cuda.Stream()
    small = pc.arc_tracks(3, 90, G, C, seed=10, bad_rows=False)
    with torch.cuda.stream(stream):
        a = _device_plan(idg, *small, stream=stream)
        b = _device_plan(idg, *small, stream=stream)
        assert a[0].tobytes() == b[0].tobytes()
        assert a[1].tobytes() == b[1].tobytes()
        _agree(idg, *small, stream=stream)
        _agree(idg, *tracks, stream=stream)         # larger B, same stream
        _agree(idg, *small, stream=stream)
    idg.release_workspaces(stream)


def test_extent_checks(idg, tracks):
    import torch
    uvw, bl, wn = (torch.from_numpy(a).cuda() for a in tracks)
    with pytest.raises(ValueError):
        idg.plan_launch(G, S, pc.IMAGE_SIZE, 0.0, uvw, bl[:5], wn, K)
    with pytest.raises(ValueError):
        idg.plan_launch(G, S, pc.IMAGE_SIZE, 0.0, uvw, bl, wn, K,
                        metadata=torch.zeros((4, 9), dtype=torch.int32,
                                             device="cuda"), capacity=5)
    with pytest.raises(idg.IdgError):
        idg.plan_launch(G, S, pc.IMAGE_SIZE, 0.0, uvw, bl, wn, S)
    md, counts = idg.plan_launch(G, S, pc.IMAGE_SIZE, 0.0, uvw, bl, wn, K)
    assert tuple(md.shape) == (12 * 300, 9) and md.dtype == torch.int32
    assert tuple(counts.shape) == (2,) and counts.dtype == torch.int32


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def test_on_cell_visibilities_end_to_end(idg, oracle_lib):
    """plan_launch -> counts[0] -> grid_onto on the device against the
    oracle pipeline under the same plan; the peak is the histogram's."""
    import torch
    o, case = pc.ONCELL, pc.oncell_case()
    t = {k: torch.from_numpy(case[k]).cuda() for k in
         ("uvw", "baselines", "wn", "vis", "aterms", "spheroidal")}
    md, counts = idg.plan_launch(o["G"], o["S"], o["image_size"], 0.0,
                                 t["uvw"], t["baselines"], t["wn"], o["K"],
                                 o["Tmax"])
    ns, dropped = (int(v) for v in counts.cpu())
    assert dropped == 0 and ns >= 2 * o["B"]
    md = md[:ns].contiguous()
    grid = torch.zeros((1, 4, o["G"], o["G"], 2), dtype=torch.float32,
                       device="cuda")
    idg.grid_onto(ns, o["G"], o["S"], o["image_size"], 0.0, 1,
                  case["nr_stations"], t["uvw"], t["wn"], t["vis"],
                  t["spheroidal"], t["aterms"], md, grid)
    got = pl.to_complex(grid.cpu().numpy())
    md_host = md.cpu().numpy().view(idg.METADATA_DTYPE).reshape(-1)
    ref = pc.oncell_grid_through_the_oracle(oracle_lib, case, md_host)
    rel = _rel(got, ref)
    print(f"grid vs the oracle pipeline: {rel:.3e}")
    assert rel < 1e-5
    assert case["hist"].ravel()[np.argmax(np.abs(got[0, 0]))] == \
        case["hist"].max()
    assert np.argmax(np.abs(got[0, 0])) == np.argmax(np.abs(ref[0, 0]))


def test_multi_channel_subgrids_under_the_device_plan(idg, oracle_lib, tracks):
    """The device gridder under the device plan against oracle.gridder under
    the host plan, the project's parity metric and bar."""
    import torch
    uvw, bl, wn = tracks
    B, T = uvw.shape[:2]
    st = int(bl.max()) + 1
    rng = np.random.default_rng(12)
    vis = rng.normal(size=(B * T, C, 4, 2)).astype(np.float32)
    at = rng.normal(size=(1, st, S, S, 4, 2)).astype(np.float32)
    x = np.linspace(-1, 1, S, dtype=np.float32)
    sph = np.ascontiguousarray(np.outer(1 - x * x, 1 - x * x))
    ref_md, _ = idg.plan(G, S, pc.IMAGE_SIZE, 0.0, uvw, bl, wn, K)
    want = np.zeros((ref_md.size, 4, S, S, 2), np.float32)
    oracle_lib.gridder(ref_md.size, G, S, pc.IMAGE_SIZE, 0.0, C, st, uvw, wn,
                       vis, sph, at, ref_md, want, nthreads=8)
    t_uvw, t_wn = torch.from_numpy(uvw).cuda(), torch.from_numpy(wn).cuda()
    md, counts = idg.plan_launch(G, S, pc.IMAGE_SIZE, 0.0, t_uvw,
                                 torch.from_numpy(bl).cuda(), t_wn, K)
    ns = int(counts[0])
    assert ns == ref_md.size
    sg = torch.zeros((ns, 4, S, S, 2), dtype=torch.float32, device="cuda")
    idg.gridder_launch(ns, G, S, pc.IMAGE_SIZE, 0.0, C, st, t_uvw, t_wn,
                       torch.from_numpy(vis).cuda(),
                       torch.from_numpy(sph).cuda(),
                       torch.from_numpy(at).cuda(), md[:ns].contiguous(), sg,
                       validate=True)
    err = oracle_lib.check_error(sg.cpu().numpy(), want)[0]
    print(f"gridder under the device plan vs the oracle: {err:.3e}")
    assert err <= TOLERANCE
