"""The host entry of Clark CLEAN (idg_clark) against the numpy
restatement of its contract in clark_cases.py: every output compared as bytes,
guard rows included; then the three properties the contract promises, the
refusals and what each case is for.  No device needed."""
import ctypes

import numpy as np
import pytest

import clark_cases as kc
import clean_cases as cc

F = np.float32


@pytest.fixture(scope="module")
def idg():
    import idg_amd
    return idg_amd


_runs = {}


def _run(idg, name):
    """(case, host buffers, restatement's buffers, its trace), made once."""
    if name not in _runs:
        c = kc.CASES[name]()
        trace = []
        want = kc.run_restatement(c, trace)
        _runs[name] = (c, kc.run_host(idg, c), want, trace)
    return _runs[name]


def _inner(b):
    return (b["residual"][1:-1], b["model"][1:-1], b["components"][1:-1],
            b["state"][0])


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_host_entry_is_the_restatement(idg, name):
    c, got, want, trace = _run(idg, name)
    st = got["state"][0]
    print(f"{name}: " + ", ".join(f"{k} {st[k]!r}" for k in kc.STATE.names))
    print("  candidates per round", [r["index"].size for r in trace],
          "components per round", [r["n1"] - r["n0"] for r in trace])
    assert kc.same_bytes(got, want) == []
    assert kc.guards_intact(got)


def test_dtypes_are_the_abis(idg):
    assert idg.CLARK_STATE_DTYPE == kc.STATE
    assert kc.STATE.itemsize == 36
    assert ctypes.sizeof(idg.ClarkParamsStruct) == 44
    assert idg.abi_version() == 1


# ---- the three properties ------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_a_same_residual_as_hogbom_on_the_same_list(idg, name):
    c, got, _, _ = _run(idg, name)
    res, _, comps, st = _inner(got)
    want = kc.hogbom_residual(c, comps[:st["n_components"]])
    assert res.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_b_candidates_agree_with_the_residual(idg, name):
    """On the restatement, whose bytes the host entry's are: after every
    round's apply (a one-round call from the state before it), the residual
    at the candidates is their final list value."""
    c = kc.CASES[name]()
    b = kc.buffers(c)
    rounds = 0
    for _ in range(sum(c["chunks"])):
        trace = []
        kc.restate(b["residual"][1:-1], c["psf"], b["model"][1:-1], c["mask"],
                   b["components"][1:-1], b["state"], nr_rounds=1,
                   trace=trace, **kc.params(c))
        for r in trace:
            rounds += 1
            at = b["residual"][1:-1].ravel()[r["index"]]
            assert at.tobytes() == r["value"].tobytes()
    assert kc.same_bytes(b, _run(idg, name)[2]) == []
    assert rounds > 0 or name == "flat"


CLAIM_C = sorted(n for n in kc.CASES if kc.CASES[n]()["claims_c"])


@pytest.mark.parametrize("name", CLAIM_C)
def test_c_same_components_as_idg_clean(idg, name):
    """The premise first, on the restatement: at every component taken, the
    whole residual's peak was the list's.  Then idg_clean from the same
    inputs.  It runs n_components iterations where Clark's reason is 0, and
    one more where it is not: that iteration takes the stop decision (below
    the level, or components full) that Clark took, and no component."""
    c, got, _, trace = _run(idg, name)
    taken = [x for r in trace for x in r["peak_listed"]]
    res, model, comps, st = _inner(got)
    n = int(st["n_components"])
    assert len(taken) == n and all(taken)
    assert st["reason"] in (0, 1, 3)
    h = cc.buffers(c)
    idg.clean(h["residual"][1:-1], c["psf"], h["model"][1:-1], c["mask"],
              nr_iterations=n + (1 if st["reason"] != 0 else 0),
              components=h["components"][1:-1], state=h["state"],
              **cc.params(c))
    hres, hmodel, hcomps, hst = _inner(h)
    assert res.tobytes() == hres.tobytes()
    assert model.tobytes() == hmodel.tobytes()
    assert comps.tobytes() == hcomps.tobytes()
    assert tuple(st)[:6] == tuple(hst)
    assert n > 0


def test_c_is_not_claimed_where_the_peak_leaves_the_list(idg):
    """The one case without the premise: it fails there, the components
    differ from idg_clean's, and the run still ends below the threshold."""
    c, got, _, trace = _run(idg, "peak_leaves_the_list")
    assert not c["claims_c"]
    taken = [x for r in trace for x in r["peak_listed"]]
    assert not all(taken)
    res, model, comps, st = _inner(got)
    n = int(st["n_components"])
    assert st["reason"] == 1 and 0 < n < c["max_components"]
    assert st["peak"] <= st["level"] == F(c["threshold"])
    h = cc.buffers(c)
    idg.clean(h["residual"][1:-1], c["psf"], h["model"][1:-1], c["mask"],
              nr_iterations=n, components=h["components"][1:-1],
              state=h["state"], **cc.params(c))
    first = taken.index(False)
    hcomps = h["components"][1:-1]
    assert comps[:first].tobytes() == hcomps[:first].tobytes()
    assert comps[first] != hcomps[first]


# ---- continuing, refreshing ------------------------------------------------------
@pytest.mark.parametrize("name,chunks", [("low", (1, 1, 1, 1, 1, 1)),
                                         ("low", (2, 4)),
                                         ("many", (1, 5)),
                                         ("three_iterations_per_round",
                                          (9,)),
                                         ("two_calls_of_three", (6,))])
def test_k_calls_of_n_rounds_are_one_call(idg, name, chunks):
    c, got, _, _ = _run(idg, name)
    assert sum(chunks) == sum(c["chunks"])
    assert kc.same_bytes(kc.run_host(idg, c, chunks), got) == []


def test_zero_rounds_only_refresh_the_peak(idg):
    c = kc.CASES["low"]()
    b, before = kc.run_host(idg, c, (0,)), kc.buffers(c)
    res, model, comps, st = _inner(b)
    assert st["peak"] == np.abs(c["residual"]).max()
    assert st["peak_index"] == np.abs(c["residual"]).argmax()
    st["peak"], st["peak_index"] = 0, 0
    assert kc.same_bytes(b, before) == []
    # and after rounds: the call changes no other byte
    b = kc.run_host(idg, c, (2,))
    mid = {k: v.copy() for k, v in b.items()}
    mid["state"]["peak"], mid["state"]["peak_index"] = -1, 77
    again = {k: v.copy() for k, v in mid.items()}
    idg.clark(again["residual"][1:-1], c["psf"], again["model"][1:-1],
              nr_rounds=0, components=again["components"][1:-1],
              state=again["state"], **kc.params(c))
    assert kc.same_bytes(again, b) == []


def test_all_rounds_by_default(idg):
    """nr_rounds=None: rounds until a reason is set."""
    c, got, _, _ = _run(idg, "low")
    b = kc.buffers(c)
    idg.clark(b["residual"][1:-1], c["psf"], b["model"][1:-1],
              components=b["components"][1:-1], state=b["state"],
              **kc.params(c))
    assert kc.same_bytes(b, got) == []
    with pytest.raises(ValueError):
        idg.clark(b["residual"][1:-1], c["psf"],
                  **dict(kc.params(c), iterations_per_round=0))


# ---- what each case is for ----------------------------------------------------
def test_low_stops_below_the_threshold(idg):
    c, got, _, trace = _run(idg, "low")
    st = _inner(got)[3]
    assert st["reason"] == 1 and st["level"] == F(0.05)
    assert st["peak"] <= st["level"] and st["n_components"] > 0
    # the last round begun is the one that found the peak below the level
    assert st["rounds"] == len(trace) + 1 <= 6
    assert all(r["tbits"] % (1 << kc.BIN_SHIFT) != 0 for r in trace)


def test_low_cap_is_bounded_by_the_histogram(idg):
    """64 candidates at most: the limit is a bin's edge (bits a multiple of
    2^19) in every round whose qualifying pixels outnumber them."""
    c, got, _, trace = _run(idg, "low_cap")
    edge = [r["tbits"] % (1 << kc.BIN_SHIFT) == 0 for r in trace]
    assert len(edge) > 2 and all(edge[:-1]) and not edge[-1]
    assert all(r["index"].size <= 64 for r in trace)
    for r, at_edge in zip(trace, edge):
        # a limit one bin lower would have listed more than 64
        assert (r["one_bin_lower"] > 64) == at_edge
    st = _inner(got)[3]
    limit = np.array([st["round_limit"]]).view(np.uint32)[0]
    assert limit == trace[-1]["tbits"]


def test_many_gives_a_thread_more_than_one_candidate(idg):
    _, got, _, trace = _run(idg, "many")
    assert 1024 < trace[0]["index"].size <= 4096
    assert _inner(got)[3]["reason"] == 1


def test_flat_has_no_candidate_and_writes_nothing(idg):
    c, got, _, trace = _run(idg, "flat")
    res, model, comps, st = _inner(got)
    assert trace == [] and (st["reason"], st["n_components"]) == (4, 0)
    assert (st["n_candidates"], st["rounds"]) == (0, 1)
    # the one occupied bin holds 1024 pixels, more than 16: b* = 4096
    assert np.array([st["round_limit"]]).view(np.uint32)[0] == 1 << 31
    assert res.tobytes() == c["residual"].tobytes()
    assert not model.any() and not comps["value"].any()
    assert (st["peak"], st["peak_index"]) == (1.0, 0)


def test_border_and_corner_components(idg):
    c, got, _, _ = _run(idg, "border_and_corners")
    comps, st = _inner(got)[2:]
    at = {(int(y), int(x)) for y, x, _ in comps[:st["n_components"]]}
    assert {(0, 0), (63, 63), (0, 63), (63, 0), (31, 0), (0, 30)} <= at


def test_ties_go_to_the_lower_index(idg):
    c, got, _, _ = _run(idg, "tie_plus_minus")
    assert c["residual"][8, 8] == -4.0 and c["residual"][20, 30] == 4.0
    assert c["residual"][40, 40] == 4.0
    comps = _inner(got)[2]
    assert [tuple(r)[:2] for r in comps[:3]] == [(8, 8), (20, 30), (40, 40)]
    assert comps[0]["value"] < 0 < comps[1]["value"]


def test_nan_is_never_listed_nor_altered_elsewhere(idg):
    c, got, _, trace = _run(idg, "nan_pixels")
    res, model, comps, st = _inner(got)
    nans = {30 * 64 + 30, 10 * 64 + 12, 0}
    assert set(np.flatnonzero(np.isnan(res))) == nans
    assert all(nans.isdisjoint(r["index"].tolist()) for r in trace)
    assert np.isfinite(st["peak"]) and st["n_components"] > 0
    # (10, 12) lies inside the patch of the source at (10, 10): it is
    # subtracted from, and stays a NaN


def test_mask_limits_the_candidates_only(idg):
    c, got, _, trace = _run(idg, "mask_hides_the_peak")
    res, model, comps, st = _inner(got)
    assert np.abs(c["residual"]).argmax() == 11 * 96 + 27
    assert all(c["mask"].ravel()[r["index"]].all() for r in trace)
    assert all(c["mask"][y, x] != 0 for y, x, _ in comps[:st["n_components"]])
    assert np.any((res != c["residual"]) & (c["mask"] == 0))
    assert c["mask"].ravel()[st["peak_index"]] != 0


def test_model_accumulates_onto_the_start_model(idg):
    c, got, _, _ = _run(idg, "start_model")
    _, model, comps, st = _inner(got)
    want = c["model"].copy()
    for y, x, v in comps[:st["n_components"]]:
        want[y, x] = F(want[y, x] + v)
    assert model.tobytes() == want.tobytes()


def test_components_full_in_mid_round(idg):
    c, got, _, trace = _run(idg, "components_full_mid_round")
    st = _inner(got)[3]
    assert (st["reason"], st["n_components"]) == (3, 30)
    # the round that filled them had taken some, and they were applied
    assert 0 < trace[-1]["n1"] - trace[-1]["n0"] < 30
    assert trace[-1]["n1"] - trace[-1]["n0"] < c["iterations_per_round"]


@pytest.mark.parametrize("name,per", [("one_iteration_per_round", 1),
                                      ("three_iterations_per_round", 3)])
def test_iterations_per_round_bound_a_round(idg, name, per):
    c, got, _, trace = _run(idg, name)
    st = _inner(got)[3]
    assert [r["n1"] - r["n0"] for r in trace] == [per] * sum(c["chunks"])
    assert (st["reason"], st["rounds"]) == (0, sum(c["chunks"]))


# ---- invalid arguments leave every buffer as it was ---------------------------
def _call(idg, c, b, params=None, **null):
    """idg_clark on buffers() with a raw parameter struct."""
    p = idg.ClarkParamsStruct(ctypes.sizeof(idg.ClarkParamsStruct), c["G"],
                              c["Gp"], c["max_components"], 2,
                              c["iterations_per_round"], c["max_candidates"],
                              c["gain"], c["threshold"], c["cycle_fraction"],
                              c["select_fraction"])
    raw = bytearray(bytes(p))
    if params is not None:
        raw = params(p, raw)
    blob = (ctypes.c_char * len(raw)).from_buffer(raw)
    ptr = {"residual": b["residual"][1:-1], "psf": c["psf"],
           "model": b["model"][1:-1], "components": b["components"][1:-1],
           "state": b["state"]}
    args = [None if k in null else v.ctypes.data_as(ctypes.c_void_p)
            for k, v in ptr.items()]
    from idg_amd._lib import lib
    return lib.idg_clark(ctypes.cast(blob, ctypes.c_void_p), args[0], args[1],
                         None, *args[2:])


def _with(**fields):
    def edit(p, raw):
        for k, v in fields.items():
            setattr(p, k, v)
        return bytearray(bytes(p))
    return edit


def _grown(p, raw):
    p.struct_size += 4
    return bytearray(bytes(p)) + b"\x01\x00\x00\x00"


INVALID = {
    "struct_size_0": _with(struct_size=0),
    "struct_size_odd": _with(struct_size=42),
    "byte_past_the_known_fields": _grown,
    "grid_size_0": _with(grid_size=0, psf_size=0),
    "grid_size_too_large": _with(grid_size=16385),
    "psf_size_0": _with(psf_size=0),
    "psf_larger_than_grid": _with(psf_size=97),
    "gain_nan": _with(gain=float("nan")),
    "gain_inf": _with(gain=float("inf")),
    "threshold_inf": _with(threshold=float("inf")),
    "threshold_negative": _with(threshold=-1.0),
    "cycle_fraction_nan": _with(cycle_fraction=float("nan")),
    "cycle_fraction_negative": _with(cycle_fraction=-0.5),
    "max_components_negative": _with(max_components=-1),
    "nr_rounds_negative": _with(nr_rounds=-1),
    "iterations_per_round_negative": _with(iterations_per_round=-1),
    "select_fraction_nan": _with(select_fraction=float("nan")),
    "select_fraction_negative": _with(select_fraction=-0.1),
    "select_fraction_above_1": _with(select_fraction=1.5),
    "max_candidates_0": _with(max_candidates=0),
    "max_candidates_too_many": _with(max_candidates=16385),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_parameters(idg, name):
    c = kc.CASES["low"]()
    b, before = kc.buffers(c), kc.buffers(c)
    assert _call(idg, c, b, INVALID[name]) == -1     # IDG_E_INVALID_ARGUMENT
    assert kc.same_bytes(b, before) == []


@pytest.mark.parametrize("null", ["residual", "psf", "model", "components",
                                  "state"])
def test_null_buffer(idg, null):
    c = kc.CASES["low"]()
    b, before = kc.buffers(c), kc.buffers(c)
    assert _call(idg, c, b, **{null: True}) == -1
    assert kc.same_bytes(b, before) == []


@pytest.mark.parametrize("n", [-1, 1001])
def test_state_out_of_range(idg, n):
    c = kc.CASES["low"]()
    b, before = kc.buffers(c), kc.buffers(c)
    b["state"]["n_components"] = before["state"]["n_components"] = n
    assert _call(idg, c, b) == -1
    assert kc.same_bytes(b, before) == []
    with pytest.raises(idg.IdgError):
        idg.clark(b["residual"][1:-1], c["psf"], b["model"][1:-1],
                  state=b["state"], components=b["components"][1:-1],
                  **kc.params(c))


def test_the_valid_struct_and_a_larger_one_of_zeros_are_accepted(idg):
    c = kc.CASES["low"]()
    b = kc.buffers(c)
    assert _call(idg, c, b) == 0
    assert b["state"][0]["rounds"] == 2

    def grown(p, raw):
        p.struct_size += 4
        return bytearray(bytes(p)) + bytes(4)
    assert _call(idg, c, b, grown) == 0
    assert b["state"][0]["rounds"] == 4


def test_select_fraction_and_max_candidates_at_their_ends(idg):
    """select_fraction 0 and 1 and max_candidates 1 and 16384 are inside the
    ranges.  At select_fraction 1 the limit lies one bit above the peak: no
    candidate."""
    c = kc.CASES["low"]()
    for edit, reason in ((dict(select_fraction=0.0), 1),
                         (dict(select_fraction=1.0), 4),
                         (dict(max_candidates=16384), 1),
                         (dict(max_candidates=1), None)):
        d = dict(c, **edit)
        got, want = kc.run_host(idg, d), kc.run_restatement(d)
        assert kc.same_bytes(got, want) == []
        if reason is not None:
            assert got["state"][0]["reason"] == reason


def test_a_crowded_level_bin_leaves_no_candidate(idg):
    c, got, _, trace = _run(idg, "peak_in_the_levels_bin")
    res, model, comps, st = _inner(got)
    assert [r["n1"] - r["n0"] for r in trace] == [1]
    assert tuple(comps[0]) == (20, 11, 5.0) and st["level"] == F(1.01)
    assert (st["reason"], st["rounds"], st["n_components"]) == (4, 2, 1)
    assert st["peak"] == F(1.02) > st["level"]
    # the level's bin holds the peak, and more pixels than the list may
    edges = kc.magnitude_bits(F([1.01, 1.02])) >> kc.BIN_SHIFT
    assert edges[0] == edges[1]
    assert (kc.magnitude_bits(res) >> kc.BIN_SHIFT == edges[0]).sum() > 16
    assert (res > st["level"]).sum() == 10 <= 16
    assert np.array([st["round_limit"]]).view(np.uint32)[0] == 1 << 31
