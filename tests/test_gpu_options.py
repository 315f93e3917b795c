"""Per-call launch options on the GPU (idg_amd.Options, the idg_*_opts entries)
and the auto gridder (Options(gridder="auto")).

A mode chosen by argument is bit for bit the mode chosen by its environment
variable, and wins over a contrary variable.  An auto launch writes, for every
subgrid above the threshold, the bits of an ordered launch of the same batch
and, for every other subgrid, the bits of a default launch in the same kernel
form; it leaves the stream's workspaces fit for the next launch.
Run on the GPU box: -m gpu.
"""
import contextlib
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, TOLERANCE

pytestmark = pytest.mark.gpu

BAR_C256 = 5e-6   # tests/test_gpu_ordered.py: the ordered kernel at C = 256
MODE_VARS = ("IDG_GRIDDER_IMPL", "IDG_DEGRIDDER_IMPL", "IDG_PREC",
             "IDG_KERNEL_FORM", "IDG_GRID_FFT", "IDG_AUTO_SLICES")


@pytest.fixture(scope="module")
def idg():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import idg_amd
    return idg_amd


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for v in MODE_VARS:
        monkeypatch.delenv(v, raising=False)


@contextlib.contextmanager
def _env(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Batch:
    """One generated batch, resident on the device."""

    def __init__(self, idg, st, ts, T, C, G, S, w_step=0.0, nr_timesteps=None,
                 w_terms=False):
        import torch
        a = idg.generate(st, ts, T, C, G, S, nthreads=8)
        md = a["metadata"].copy()
        if nr_timesteps is not None:
            md["nr_timesteps"] = np.resize(
                np.asarray(nr_timesteps, np.int32), md.size)
        if w_terms:
            rng = np.random.default_rng(3)
            a["uvw"][..., 2] = rng.uniform(-200, 200, a["uvw"].shape[:2])
            md["z"] = rng.integers(-3, 4, md.size)
        a["metadata"] = md
        self.idg, self.a, self.md, self.S, self.C = idg, a, md, S, C
        self.ns = md.size
        self.params = (md.size, G, S, idg.IMAGE_SIZE, w_step, C, st)
        self.dev = {k: torch.from_numpy(v).cuda() for k, v in a.items()
                    if k not in ("metadata", "frequencies")}
        self.dev["metadata"] = torch.from_numpy(
            md.view(np.int32).reshape(-1, 9).copy()).cuda()

    def _args(self, vis=None):
        d = self.dev
        return (*self.params, d["uvw"], d["wavenumbers"],
                d["visibilities"] if vis is None else vis, d["spheroidal"],
                d["aterms"], d["metadata"])

    def grid_t(self, options=None, fft=False, fill=7.25):
        """Device gridder launch into a poisoned tensor (left on device)."""
        import torch
        out = torch.full_like(self.dev["subgrids"], fill)
        launch = (self.idg.gridder_fft_launch if fft
                  else self.idg.gridder_launch)
        launch(*self._args(), out, options=options)
        return out

    def grid(self, options=None, fft=False, fill=7.25):
        import torch
        out = self.grid_t(options, fft, fill)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.int32)

    def degrid(self, options=None):
        import torch
        vis = torch.full_like(self.dev["visibilities"], -3.5)
        self.idg.degridder_launch(*self._args(vis), self.dev["subgrids"],
                                  options=options)
        torch.cuda.synchronize()
        return vis.cpu().numpy().view(np.int32)

    def grid_host(self, options=None):
        a = self.a
        out = np.full((self.ns, 4, self.S, self.S, 2), 7.25, np.float32)
        self.idg.c_run_gridder(*self.params, a["uvw"], a["wavenumbers"],
                               a["visibilities"], a["spheroidal"],
                               a["aterms"], self.md, out, options=options)
        return out.view(np.int32)

    def degrid_host(self, options=None):
        a = self.a
        vis = np.full_like(a["visibilities"], -3.5)
        self.idg.c_run_degridder(*self.params, a["uvw"], a["wavenumbers"],
                                 vis, a["spheroidal"], a["aterms"], self.md,
                                 a["subgrids"], options=options)
        return vis.view(np.int32)


def _same(got, want, what):
    assert got.shape == want.shape
    assert np.array_equal(got, want), \
        f"{what}: {int((got != want).sum())} of {got.size} words differ"


# -- 1: mode by argument = mode by environment --------------------------------
@pytest.fixture(scope="module", params=[32, 33])
def small(idg, request):
    return Batch(idg, 3, 1, 16, 16, 512, request.param)


GRIDDER_IMPLS = ("default", "valu", "sequential", "ordered")
DEGRIDDER_IMPLS = ("default", "sequential")


def _contrary(impl):
    return "sequential" if impl != "sequential" else "default"


def test_gridder_impl_by_option_is_impl_by_environment(idg, small):
    outs = {}
    for impl in GRIDDER_IMPLS:
        with _env(IDG_GRIDDER_IMPL=impl):
            by_env, by_env_host = small.grid(), small.grid_host()
        opt = idg.Options(gridder=impl)
        _same(small.grid(opt), by_env, f"device, {impl}")
        _same(small.grid_host(opt), by_env_host, f"host, {impl}")
        with _env(IDG_GRIDDER_IMPL=_contrary(impl)):
            _same(small.grid(opt), by_env, f"device, {impl} over variable")
            _same(small.grid_host(opt), by_env_host,
                  f"host, {impl} over variable")
        outs[impl] = by_env
    # the impls are told apart by their bits, so the checks above can fail
    assert not np.array_equal(outs["default"], outs["sequential"])
    assert not np.array_equal(outs["default"], outs["ordered"])
    assert not np.array_equal(outs["sequential"], outs["ordered"])


def test_degridder_impl_by_option_is_impl_by_environment(idg, small):
    outs = {}
    for impl in DEGRIDDER_IMPLS:
        with _env(IDG_DEGRIDDER_IMPL=impl):
            by_env, by_env_host = small.degrid(), small.degrid_host()
        opt = idg.Options(degridder=impl)
        _same(small.degrid(opt), by_env, f"device, {impl}")
        _same(small.degrid_host(opt), by_env_host, f"host, {impl}")
        with _env(IDG_DEGRIDDER_IMPL=_contrary(impl)):
            _same(small.degrid(opt), by_env, f"device, {impl} over variable")
            _same(small.degrid_host(opt), by_env_host,
                  f"host, {impl} over variable")
        outs[impl] = by_env
    assert not np.array_equal(outs["default"], outs["sequential"])


# -- 2: kernel_form and fft_fusion by option ----------------------------------
def test_kernel_form_and_fft_fusion_by_option(idg, small):
    for form, other in (("combined", "split"), ("split", "combined")):
        with _env(IDG_KERNEL_FORM=form):
            g_env, d_env = small.grid(), small.degrid()
        opt = idg.Options(kernel_form=form)
        _same(small.grid(opt), g_env, f"gridder, {form}")
        _same(small.degrid(opt), d_env, f"degridder, {form}")
        with _env(IDG_KERNEL_FORM=other):
            _same(small.grid(opt), g_env, f"gridder, {form} over variable")
            _same(small.degrid(opt), d_env, f"degridder, {form} over variable")
    for fusion, var, other in ((False, "0", "1"), (True, "1", "0")):
        with _env(IDG_GRID_FFT=var):
            f_env = small.grid(fft=True)
        opt = idg.Options(fft_fusion=fusion)
        _same(small.grid(opt, fft=True), f_env, f"fft_fusion={fusion}")
        with _env(IDG_GRID_FFT=other):
            _same(small.grid(opt, fft=True), f_env,
                  f"fft_fusion={fusion} over variable")
        assert idg.kernel_name("gridder", 32, 16, opt) == "gridder_mi355x_s32"


def test_precision_by_option(idg, small):
    with _env(IDG_PREC="0"):
        want = small.grid()
    _same(small.grid(idg.Options(precision=0)), want, "precision 0")
    with _env(IDG_PREC="1"):
        _same(small.grid(idg.Options(precision=0)), want,
              "precision 0 over variable")


# -- 3: auto, small threshold -------------------------------------------------
RAGGED = (0, 3, 4, 5, 16)
AUTO_CASES = [(S, form, False) for S in (32, 64, 33)
              for form in ("combined", "split")] + [(32, "split", True)]


@pytest.fixture(scope="module", params=AUTO_CASES,
                ids=lambda c: f"S{c[0]}-{c[1]}" + ("-wstep" if c[2] else ""))
def ragged(idg, request):
    """12 subgrids, nr_timesteps cycling 0, 3, 4, 5, 16 at C = 16, and the
    default (in the case's kernel form) and ordered outputs, computed once."""
    S, form, w = request.param
    b = Batch(idg, 4, 2, 16, 16, 512, S, w_step=2.5 if w else 0.0,
              nr_timesteps=RAGGED, w_terms=w)
    assert b.ns == 12
    default = b.grid(idg.Options(gridder="default", kernel_form=form))
    ordered = b.grid(idg.Options(gridder="ordered"))
    for x in (default, ordered):
        x.setflags(write=False)
    return b, form, default, ordered


def _check_per_subgrid(auto, sel, default, ordered, what):
    for s in range(auto.shape[0]):
        want, name = ((ordered, "ordered") if sel[s] else (default, "default"))
        _same(auto[s], want[s], f"{what}: subgrid {s} against {name}")


def test_auto_small_threshold(idg, ragged):
    b, form, default, ordered = ragged
    opt = idg.Options(gridder="auto", kernel_form=form, auto_threshold=64)
    sel = idg.auto_selected(b.md, 16, opt)
    T = b.md["nr_timesteps"]
    assert np.array_equal(sel, (T * 16 > 64).astype(np.uint8))
    assert 0 < sel.sum() < sel.size
    # the two kernels differ on the selected subgrids, so a swap would show
    assert all(not np.array_equal(default[s], ordered[s])
               for s in np.flatnonzero(sel))
    before = b.grid(idg.Options(gridder="default", kernel_form=form))
    auto = b.grid(opt)
    # straight after the auto launch, same stream: the workspaces it shares
    after_t = b.grid_t(idg.Options(gridder="default", kernel_form=form))
    again = b.grid(opt, fill=-1.0)
    after = after_t.cpu().numpy().view(np.int32)
    _check_per_subgrid(auto, sel, default, ordered, "auto")
    _same(again, auto, "a second auto launch")
    _same(before, default, "default before auto")
    _same(after, default, "default straight after auto")


def test_auto_threshold_extremes(idg, ragged):
    b, form, default, ordered = ragged
    above = idg.Options(gridder="auto", kernel_form=form, auto_threshold=256)
    assert not idg.auto_selected(b.md, 16, above).any()
    _same(b.grid(above), default, "a threshold above every product")
    one = idg.Options(gridder="auto", kernel_form=form, auto_threshold=1)
    assert np.array_equal(idg.auto_selected(b.md, 16, one),
                          b.md["nr_timesteps"] > 0)
    _same(b.grid(one), ordered, "threshold 1")


def test_auto_by_environment_and_host_entry(idg, ragged):
    b, form, default, ordered = ragged
    opt = idg.Options(gridder="auto", kernel_form=form, auto_threshold=64)
    sel = idg.auto_selected(b.md, 16, opt)
    auto = b.grid(opt)
    with _env(IDG_GRIDDER_IMPL="auto"):
        _same(b.grid(idg.Options(kernel_form=form, auto_threshold=64)), auto,
              "IDG_GRIDDER_IMPL=auto")
    _same(b.grid_host(opt), auto, "c_run_gridder(options=auto)")
    _check_per_subgrid(auto, sel, default, ordered, "auto")


@pytest.mark.parametrize("slices", [1, 3, 4])
def test_auto_slicing_keeps_the_bits(idg, ragged, slices):
    """The ordered pass with another number of workgroups per subgrid (the
    measurement knob of tools/debug/auto_rate.py): the same bits."""
    b, form, default, ordered = ragged
    opt = idg.Options(gridder="auto", kernel_form=form, auto_threshold=1)
    with _env(IDG_AUTO_SLICES=str(slices)):
        _same(b.grid(opt), ordered, f"{slices} slices per subgrid")


# -- 4: auto, the library's threshold -----------------------------------------
def test_auto_library_threshold_c256(idg, oracle_lib):
    b = Batch(idg, 3, 1, 128, 256, 1024, 32, nr_timesteps=(64, 65, 128))
    assert b.ns == 3
    opt = idg.Options(gridder="auto")
    sel = idg.auto_selected(b.md, 256, opt)
    assert list(sel) == [0, 1, 1]
    default = b.grid(idg.Options(gridder="default"))
    ordered = b.grid(idg.Options(gridder="ordered"))
    auto = b.grid(opt)
    _check_per_subgrid(auto, sel, default, ordered, "auto, C = 256")
    a = b.a
    want = np.zeros((3, 4, 32, 32, 2), np.float32)
    oracle_lib.gridder(*b.params, a["uvw"], a["wavenumbers"],
                       a["visibilities"], a["spheroidal"], a["aterms"], b.md,
                       want, nthreads=min(16, os.cpu_count() or 1))
    got = auto.view(np.float32)
    pick = sel.astype(bool)
    e_sel = oracle_lib.check_error(np.ascontiguousarray(got[pick]),
                                   np.ascontiguousarray(want[pick]))[0]
    e_rest = oracle_lib.check_error(np.ascontiguousarray(got[~pick]),
                                    np.ascontiguousarray(want[~pick]))[0]
    e_all = oracle_lib.check_error(got, want)[0]
    print(f"auto vs oracle at C = 256: selected {e_sel:.3e}, unselected "
          f"{e_rest:.3e}, whole batch {e_all:.3e}")
    assert e_sel <= BAR_C256
    assert e_all <= TOLERANCE


# -- 5: fusion under auto -----------------------------------------------------
@pytest.mark.parametrize("S", [32, 64])   # 32: where the default pass fuses
def test_fft_and_grid_onto_under_auto(idg, S):
    import torch
    b = Batch(idg, 4, 2, 16, 16, 512, S, nr_timesteps=RAGGED)
    opt = idg.Options(gridder="auto", auto_threshold=64)
    assert 0 < idg.auto_selected(b.md, 16, opt).sum() < b.ns
    two = b.grid_t(opt)
    idg.subgrid_fft_launch(two, +1, 1.0)
    fused = b.grid_t(opt, fft=True)
    torch.cuda.synchronize()
    assert torch.equal(fused.view(torch.int32), two.view(torch.int32))
    assert idg.kernel_name("gridder", b.S, 16, opt).startswith("gridder_auto_")
    G = b.params[1]
    d = b.dev
    grid_a = torch.zeros((1, 4, G, G, 2), dtype=torch.float32, device="cuda")
    grid_b = torch.zeros_like(grid_a)
    idg.adder_launch(G, d["metadata"], two, grid_a)
    idg.grid_onto(*b.params, d["uvw"], d["wavenumbers"], d["visibilities"],
                  d["spheroidal"], d["aterms"], d["metadata"], grid_b,
                  options=opt)
    torch.cuda.synchronize()
    assert grid_a.abs().max() > 0
    assert torch.equal(grid_a.view(torch.int32), grid_b.view(torch.int32))


# -- 6: more selected subgrids than fit the device at once --------------------
def test_auto_many_selected_subgrids(idg):
    """4,095 subgrids, all selected: the ordered pass's grid (one workgroup
    per queue position and slice, not a resident grid) covers every one."""
    b = Batch(idg, 91, 1, 2, 16, 1024, 32)
    assert b.ns == 4095
    opt = idg.Options(gridder="auto", auto_threshold=1)
    _same(b.grid(opt), b.grid(idg.Options(gridder="ordered")),
          "4,095 selected subgrids")


# -- 7: the environment route end to end --------------------------------------
def test_restated_harness_auto_c256_passes():
    path = os.path.join(REPO, "tests", "harness", "bin", "hip-gridder_mi355x")
    assert os.path.exists(path), "build the harness: make -C tests/harness"
    r = subprocess.run([path, "-c"], env=dict(
        os.environ, IDG_GRIDDER_IMPL="auto", NR_CHANNELS="256",
        IDG_QUIET="1"), capture_output=True, text=True, timeout=300)
    assert ">>> Result PASSED" in r.stdout, r.stdout[-2000:] + r.stderr
    assert r.returncode == 0


def _perf_rate(tmp_path, **env):
    import re
    path = os.path.join(REPO, "tests", "harness", "bin", "hip-gridder_mi355x")
    r = subprocess.run([path], env=dict(
        os.environ, NR_STATIONS="12", NR_TIMESLOTS="1", NR_CHANNELS="256",
        NR_WARM_UP_RUNS="1", NR_ITERATIONS="3", **env),
        capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rates = re.findall(r"([\d.]+) MVis/s", r.stdout)
    assert rates, r.stdout[-3000:]
    return float(rates[-1])


def test_perf_entry_under_auto_times_the_whole_sequence(tmp_path):
    """hip::p_run_gridder with IDG_GRIDDER_IMPL=auto at T x C = 32,768: every
    subgrid takes the ordered pass, so the reported rate is the ordered
    kernel's, several times below the default kernels' (3.3 x at a full
    batch; more on these 66 subgrids, which do not fill the
    device) -- not the rate of the default pass alone."""
    default = _perf_rate(tmp_path, IDG_GRIDDER_IMPL="default")
    auto = _perf_rate(tmp_path, IDG_GRIDDER_IMPL="auto")
    print(f"perf entry at C = 256, 66 subgrids: default {default:.1f}, "
          f"auto {auto:.1f} MVis/s")
    assert auto * 2 <= default
