"""Imaging weights on the host (idg_weight_density / _scheme / _apply; DESIGN.md
§14) against the numpy restatement of the contract in tests/weight_cases.py.
No device is needed.  Densities, imaging weights and weighted visibilities
are compared bit for bit; the two double sums within n 2^-52 relative of the
exact sum of the same terms (a sequential double sum of n non-negative terms
is within (n - 1) 2^-53 of it)."""
import ctypes

import numpy as np
import pytest

import weight_cases as wc

F = np.float32


@pytest.fixture(scope="module")
def idg():
    import idg_amd
    return idg_amd


@pytest.fixture(scope="module")
def arcs():
    return wc.planned()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _density(idg, c, **kw):
    return idg.weight_density(c["G"], c["S"], c["image_size"], c["uvw"],
                              c["wn"], c["weights"], c["md"], **kw)


def _apply(idg, c, d, ab, vis="own", **kw):
    return idg.weight_apply(c["G"], c["image_size"], c["uvw"], c["wn"],
                            c["weights"], c["md"], d, ab,
                            c["vis"] if isinstance(vis, str) else vis, **kw)


def _restated_density(c, **kw):
    return wc.density(c["G"], c["image_size"], c["uvw"], c["wn"],
                      c["weights"], c["md"], **kw)


def _restated_apply(c, d, a, b, vis="own", **kw):
    return wc.apply(c["G"], c["image_size"], c["uvw"], c["wn"], c["weights"],
                    c["md"], d, a, b,
                    c["vis"] if isinstance(vis, str) else vis, **kw)


# ---- against the restatement -------------------------------------------------
@pytest.mark.parametrize("make", [wc.planned, wc.generated, wc.one_cell],
                         ids=["planned", "generated", "one_cell"])
def test_density_is_the_restatement(idg, make):
    c = make()
    got = _density(idg, c)
    want = _restated_density(c)
    assert got.dtype == np.uint64 and got.shape == (c["G"], c["G"])
    assert want.sum() > 0
    assert np.array_equal(got, want)


def test_density_accumulates(idg, arcs):
    half = arcs["md"].size // 2
    a, b = dict(arcs, md=arcs["md"][:half]), dict(arcs, md=arcs["md"][half:])
    # (rows are indexed from the first record's baseline_offset, 0 in a plan)
    d = _density(idg, a)
    assert _density(idg, b, density=d) is d
    assert np.array_equal(d, _density(idg, arcs))


@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("scheme", wc.SCHEMES)
def test_scheme_and_apply_are_the_restatement(idg, arcs, scheme, hermitian):
    c = arcs
    d = _density(idg, c)
    ab = idg.weight_scheme(c["G"], d, scheme, 0.5, hermitian=hermitian)
    a, b = wc.scheme_ab(d, scheme, 0.5, hermitian=hermitian)
    assert ab.dtype == F and ab[0] == a
    assert wc.ulps_apart(ab[1], b) <= (1 if scheme == "briggs" else 0)
    # apply at the library's own (a, b): bit for bit
    iw, out, total = _apply(idg, c, d, ab, hermitian=hermitian)
    riw, rout, rtotal, n = _restated_apply(c, d, ab[0], ab[1],
                                           hermitian=hermitian)
    assert np.array_equal(_bits(iw), _bits(riw))
    assert np.array_equal(_bits(out), _bits(rout))
    assert rtotal > 0 and abs(total[0] - rtotal) <= n * 2.0 ** -52 * rtotal
    if scheme == "natural":
        cov = wc.cover(c["md"], iw.shape[0]) > 0
        assert np.array_equal(iw[cov], c["weights"][cov])


def test_oncell_density_is_the_histogram(idg):
    c = wc.oncell()
    d = _density(idg, c)
    assert np.array_equal(d, c["hist"].astype(np.uint64) << np.uint64(20))
    # and uniform weighting gives every occupied cell a total weight of 1
    ab = idg.weight_scheme(c["G"], d, "uniform", hermitian=False)
    iw, _, total = _apply(idg, c, d, ab, hermitian=False)
    assert abs(total[0] - np.count_nonzero(c["hist"])) < 1e-3


def test_flagged_samples(idg, arcs):
    c, where = wc.flagged(arcs)
    d = _density(idg, c)
    assert np.array_equal(d, _restated_density(c))
    # the flagged samples added nothing: the density of the clean case less
    # what those samples held there
    q, X, Y = wc.sample_q(arcs["G"], arcs["image_size"], arcs["uvw"],
                          arcs["wn"], arcs["weights"])
    less = _density(idg, arcs).copy()
    for kind, (r, ch) in where.items():
        for k in (range(arcs["C"]) if kind == "off_grid" else [ch]):
            less[Y[r, k], X[r, k]] -= q[r, k]
    assert np.array_equal(d, less)
    for scheme in wc.SCHEMES:
        ab = idg.weight_scheme(c["G"], d, scheme, 0.0)
        iw, out, _ = _apply(idg, c, d, ab)
        riw, rout, _, _ = _restated_apply(c, d, ab[0], ab[1])
        assert np.array_equal(_bits(iw), _bits(riw))
        assert np.array_equal(_bits(out), _bits(rout))
        for kind, (r, ch) in where.items():
            chans = slice(None) if kind == "off_grid" else ch
            assert not np.any(_bits(iw[r, chans])), kind
            assert not np.any(_bits(out[r, chans])), kind
        assert np.isfinite(out).all()


def test_uncovered_rows_and_in_place(idg, arcs):
    c = arcs
    cov = wc.cover(c["md"], c["weights"].shape[0]) > 0
    assert (~cov).sum() > 0 and cov.sum() > 0
    d = _density(idg, c)
    ab = idg.weight_scheme(c["G"], d, "briggs", -0.5)
    iw0 = np.full(c["weights"].shape, -7.0, F)
    out0 = np.full(c["vis"].shape, -9.0, F)
    iw, out, total = _apply(idg, c, d, ab, imaging_weights=iw0.copy(),
                            out=out0.copy())
    assert np.all(iw[~cov] == -7.0) and np.all(out[~cov] == -9.0)
    assert not np.any(iw[cov] == -7.0)
    riw, rout, _, _ = _restated_apply(c, d, ab[0], ab[1], iw=iw0, out=out0)
    assert np.array_equal(_bits(iw), _bits(riw))
    assert np.array_equal(_bits(out), _bits(rout))
    # in place: out is visibilities; uncovered rows keep their visibilities
    vis = c["vis"].copy()
    iw2, out2, total2 = _apply(idg, c, d, ab, vis=vis, out=vis)
    assert out2 is vis
    assert np.array_equal(_bits(vis[cov]), _bits(out[cov]))
    assert np.array_equal(_bits(vis[~cov]), _bits(c["vis"][~cov]))
    assert np.array_equal(_bits(iw2), _bits(
        np.where(cov[:, None], iw, F(0)).astype(F)))
    assert total2[0] == total[0]


def test_psf_input(idg, arcs):
    c = arcs
    d = _density(idg, c)
    ab = idg.weight_scheme(c["G"], d, "uniform")
    iw, out, _ = _apply(idg, c, d, ab, vis=None)
    want = np.zeros_like(out)
    want[:, :, 0, 0] = iw
    want[:, :, 3, 0] = iw
    assert np.array_equal(_bits(out), _bits(want))
    assert iw.max() > 0


# ---- hermitian ---------------------------------------------------------------
def _hand_case(cells_xy, G=64, S=32):
    """One sample of weight 1 per cell given, C = 1, on-cell (u = cell offset
    * 64 at wavenumber 2 pi, image_size 1/64), one subgrid over them all."""
    import idg_amd
    uvw = np.zeros((len(cells_xy), 3), F)
    for i, (x, y) in enumerate(cells_xy):
        uvw[i, :2] = ((x - G // 2) * 64.0, (y - G // 2) * 64.0)
    md = np.zeros(1, idg_amd.METADATA_DTYPE)
    md["nr_timesteps"] = len(cells_xy)
    md["station2"] = 1
    return dict(G=G, S=S, C=1, image_size=1.0 / 64, uvw=uvw,
                wn=np.array([2 * np.pi], F), md=md,
                weights=np.ones((len(cells_xy), 1), F),
                vis=np.ones((len(cells_xy), 1, 4, 2), F))


def test_hermitian_by_hand(idg):
    G = 64
    cells = [(32, 32), (0, 5), (7, 0), (0, 0), (40, 20), (24, 44), (40, 20),
             (10, 50)]
    c = _hand_case(cells, G)
    d = _density(idg, c)
    hist = np.zeros((G, G), np.uint64)
    for x, y in cells:
        hist[y, x] += np.uint64(1 << 20)
    assert np.array_equal(d, hist)
    ab = idg.weight_scheme(G, d, "uniform")
    iw, _, _ = _apply(idg, c, d, ab)
    D = 1.0 / iw[:, 0]          # f = w / D with w = 1
    # the centre cell is its own mirror: it counts twice
    assert D[0] == 2.0
    # row 0 and column 0 have no mirror: their own count only
    assert D[1] == 1.0 and D[2] == 1.0 and D[3] == 1.0
    # (40, 20) twice and its mirror (24, 44) once: 3 on both sides
    assert D[4] == 3.0 and D[5] == 3.0 and D[6] == 3.0
    # a lone cell whose mirror (54, 14) is empty
    assert D[7] == 1.0
    Dr = wc.D_of(d)
    assert np.array_equal(Dr[1:, 1:], Dr[1:, 1:][::-1, ::-1])
    # hermitian off: every cell its own count
    iw, _, _ = _apply(idg, c, d, ab, hermitian=False)
    assert np.array_equal(1.0 / iw[:, 0], [1, 1, 1, 1, 2, 1, 2, 1])


# ---- Briggs limits -------------------------------------------------------------
def test_briggs_on_an_empty_density_is_natural(idg, arcs):
    c = arcs
    d = np.zeros((c["G"], c["G"]), np.uint64)
    ab = idg.weight_scheme(c["G"], d, "briggs", 0.0)
    assert ab[0] == 1.0 and ab[1] == 0.0
    nat = idg.weight_scheme(c["G"], d, "natural")
    iw, _, _ = _apply(idg, c, d, ab)
    iwn, _, _ = _apply(idg, c, d, nat)
    assert np.array_equal(_bits(iw), _bits(iwn))
    cov = wc.cover(c["md"], iw.shape[0]) > 0
    assert np.array_equal(iw[cov], c["weights"][cov])


def test_briggs_limits(idg, arcs):
    """f / w = 1 / (1 + b D).  With x = b D over the covered samples:
    robust -> +inf makes x small and the ratio of two samples' f / w differs
    from natural's (1) by at most max x, plus the float32 roundings of the
    three operations behind each f, each within u = 2^-24 relative: a factor
    inside [((1 - u) / (1 + u))^3, ((1 + u) / (1 - u))^3]; robust -> -inf
    makes x large and b f / w = (1 / D) x / (1 + x) differs from uniform's
    f / w = 1 / D by a relative 1 / min x at most, times the same factor (three
    roundings behind the one, one behind the other).  x is measured from the
    case, not chosen."""
    c = arcs
    u = 2.0 ** -24
    roundings = ((1 + u) / (1 - u)) ** 3
    d = _density(idg, c)
    cov = wc.cover(c["md"], c["weights"].shape[0]) > 0
    w = c["weights"].astype(np.float64)
    live = cov[:, None] & np.ones_like(w, bool)
    uni, _, _ = _apply(idg, c, d, idg.weight_scheme(c["G"], d, "uniform"))
    D = (w / np.where(uni > 0, uni, 1))[live]          # D per sample

    ab = idg.weight_scheme(c["G"], d, "briggs", 8.0)
    iw, _, _ = _apply(idg, c, d, ab)
    x = float(ab[1]) * D
    assert 0 < x.max() < 1e-3
    r = (iw / w)[live]
    assert np.abs(r / r[0] - 1).max() <= (1 + x.max()) * roundings - 1

    ab = idg.weight_scheme(c["G"], d, "briggs", -8.0)
    iw, _, _ = _apply(idg, c, d, ab)
    x = float(ab[1]) * D
    assert x.min() > 1e3
    r = (iw / w)[live] * float(ab[1])          # -> 1 / D
    ru = (uni / w)[live]
    assert np.abs(r / ru - 1).max() <= (1 + 1 / x.min()) * roundings - 1


# ---- errors -------------------------------------------------------------------
def _raw(idg, c, params):
    """idg_weight_density through ctypes with a caller-built params blob."""
    from idg_amd._lib import lib
    d = np.zeros((c["G"], c["G"]), np.uint64)
    buf = ctypes.create_string_buffer(bytes(params), len(params))
    p = ctypes.c_void_p
    rc = lib.idg_weight_density(
        ctypes.cast(buf, p), c["md"].size, c["S"], c["C"],
        c["md"].ctypes.data_as(p), c["uvw"].ctypes.data_as(p),
        c["uvw"].shape[0], c["wn"].ctypes.data_as(p),
        c["weights"].ctypes.data_as(p), d.ctypes.data_as(p))
    return rc, d


def _blob(c, size=None, tail=b"", **over):
    from idg_amd._lib import WeightParamsStruct
    s = WeightParamsStruct()
    s.struct_size = ctypes.sizeof(s) + len(tail) if size is None else size
    s.grid_size, s.image_size = c["G"], c["image_size"]
    s.quantum_log2, s.hermitian = wc.QLOG2, 1
    for k, v in over.items():
        setattr(s, k, v)
    return bytes(s) + tail


def test_struct_size_rules(idg, arcs):
    c = arcs
    want = _restated_density(c)
    rc, d = _raw(idg, c, _blob(c))
    assert rc == 0 and np.array_equal(d, want)
    # larger, the unknown bytes zero: accepted; one of them set: refused
    rc, d = _raw(idg, c, _blob(c, tail=bytes(8)))
    assert rc == 0 and np.array_equal(d, want)
    rc, _ = _raw(idg, c, _blob(c, tail=bytes(7) + b"\x01"))
    assert rc == -1
    # smaller: the fields beyond it are zero (here quantum_log2 = 0: every
    # weight in [0.25, 4] rounds to an integer count)
    rc, d = _raw(idg, c, _blob(c, size=12))
    assert rc == 0 and np.array_equal(d, _restated_density(c, qlog2=0))
    for size in (0, 2, 6, 1 << 17):
        rc, _ = _raw(idg, c, _blob(c, size=size))
        assert rc == -1, size


def test_invalid_arguments(idg, arcs):
    c = arcs
    for over in (dict(grid_size=0), dict(grid_size=1 << 15),
                 dict(quantum_log2=-65), dict(quantum_log2=65),
                 dict(scheme=3), dict(scheme=-1), dict(robust=float("nan")),
                 dict(robust=float("inf")), dict(image_size=float("nan"))):
        rc, _ = _raw(idg, c, _blob(c, **over))
        assert rc == -1, over
    with pytest.raises(idg.IdgError) as e:
        idg.weight_scheme(c["G"], np.zeros((c["G"], c["G"]), np.uint64),
                          "briggs", float("nan"))
    assert e.value.code == -1
    with pytest.raises(idg.IdgError) as e:
        idg.weight_density(c["G"], 0, c["image_size"], c["uvw"], c["wn"],
                           c["weights"], c["md"])
    assert e.value.code == -1


def test_metadata_out_of_bounds(idg, arcs):
    c = arcs
    d = _density(idg, c)
    ab = idg.weight_scheme(c["G"], d, "natural")
    for field, value in (("time_offset", c["uvw"].shape[0] - 1),
                         ("time_offset", -1), ("nr_timesteps", -1)):
        md = c["md"].copy()
        md[field][3] = value
        bad = dict(c, md=md)
        with pytest.raises(idg.IdgError) as e:
            _density(idg, bad)
        assert e.value.code == -2
        with pytest.raises(idg.IdgError) as e:
            _apply(idg, bad, d, ab)
        assert e.value.code == -2


def test_no_subgrids_is_a_no_op(idg, arcs):
    c = dict(arcs, md=arcs["md"][:0])
    d = np.full((c["G"], c["G"]), 5, np.uint64)
    assert np.all(_density(idg, c, density=d) == 5)
    for scheme, want in (("natural", (1, 0)), ("uniform", (0, 1))):
        assert tuple(idg.weight_scheme(c["G"], d, scheme)) == want
    iw0 = np.full(c["weights"].shape, -7.0, F)
    iw, out, total = _apply(idg, c, d, np.array([1, 0], F),
                            imaging_weights=iw0, sum_weights=np.ones(1))
    assert np.all(iw == -7.0) and total[0] == 0.0


def test_a_cell_past_2_to_62_is_refused(idg):
    c = _hand_case([(40, 20)])
    G = c["G"]
    # two densities whose sum in one cell passes 2^62: what is there already,
    # and the sample this call adds
    d = np.zeros((G, G), np.uint64)
    d[20, 40] = np.uint64(2 ** 62 - 2 ** 20)
    before = d.copy()
    with pytest.raises(idg.IdgError) as e:
        _density(idg, c, density=d)
    assert e.value.code == -1 and np.array_equal(d, before)
    d[20, 40] -= np.uint64(1)
    _density(idg, c, density=d)
    assert d[20, 40] == np.uint64(2 ** 62 - 1)
    # a density that is already there is refused by every host entry
    d[20, 40] = np.uint64(2 ** 62)
    for call in (lambda: _density(idg, c, density=d),
                 lambda: idg.weight_scheme(G, d, "briggs"),
                 lambda: _apply(idg, c, d, np.array([1, 0], F))):
        with pytest.raises(idg.IdgError) as e:
            call()
        assert e.value.code == -1
