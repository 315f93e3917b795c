"""Per-call launch options (include/idg_mi355x.h idg_options_t, idg_amd.Options)
on the host: what the library selects -- kernel names and precision bits --
for every combination of option and environment variable, the struct_size
rules, and the host twin of the auto gridder's classification.  No GPU.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

import idg_amd
from idg_amd import Options, OptionsStruct
from idg_amd._lib import lib

E_INVALID = -1
SUFFIX = {32: "s32", 64: "s64", 33: "generic"}
SIZES = (32, 64, 33)
MODE_VARS = ("IDG_GRIDDER_IMPL", "IDG_DEGRIDDER_IMPL", "IDG_PREC",
             "IDG_KERNEL_FORM", "IDG_GRID_FFT")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for v in MODE_VARS:
        monkeypatch.delenv(v, raising=False)


def _zero_struct():
    o = OptionsStruct()
    o.struct_size = ctypes.sizeof(OptionsStruct)
    return o


def _names_and_bits(options):
    return [(idg_amd.kernel_name(d, S, C, options=options),
             idg_amd.precision_options(d, S, C, options=options))
            for d in ("gridder", "degridder") for S in SIZES
            for C in (16, 256)]


def _today():
    """The entries without options."""
    return [(idg_amd.kernel_name(d, S, C), idg_amd.precision_options(d, S, C))
            for d in ("gridder", "degridder") for S in SIZES
            for C in (16, 256)]


ENVS = [{}] + [{"IDG_GRIDDER_IMPL": v}
               for v in ("default", "valu", "sequential", "ordered", "auto")] \
    + [{"IDG_DEGRIDDER_IMPL": v} for v in ("default", "valu", "sequential")] \
    + [{"IDG_PREC": str(b)} for b in range(8)]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: "-".join(
    f"{k}={v}" for k, v in e.items()) or "no-variable")
def test_unset_options_are_todays_behaviour(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = _today()
    assert _names_and_bits(None) == want
    assert _names_and_bits(Options()) == want
    assert _names_and_bits(_zero_struct()) == want
    # fields beyond the caller's struct_size count as unset
    short = _zero_struct()
    short.struct_size = 4
    short.gridder_impl = 4      # not covered by struct_size = 4
    assert _names_and_bits(short) == want


def test_legacy_entries_are_the_opts_entries_with_null():
    for d in (0, 1):
        assert lib.idg_kernel_name(d, 32, 16) == \
            lib.idg_kernel_name_opts(d, 32, 16, None)
        assert lib.idg_precision_options(d, 32, 256) == \
            lib.idg_precision_options_opts(d, 32, 256, None)


GRIDDER_NAMES = {
    "default": "gridder_mi355x_{}", "valu": "gridder_mi355x_{}_valu",
    "sequential": "gridder_sequential_mi355x_{}",
    "ordered": "gridder_ordered_mi355x_{}", "auto": "gridder_auto_mi355x_{}",
}
DEGRIDDER_NAMES = {"default": "degridder_mi355x_{}",
                   "sequential": "degridder_sequential_mi355x_{}"}


@pytest.mark.parametrize("S", SIZES)
def test_names_of_every_impl(S, monkeypatch):
    for impl, pat in GRIDDER_NAMES.items():
        assert idg_amd.kernel_name("gridder", S, 16, Options(gridder=impl)) \
            == pat.format(SUFFIX[S])
    for impl, pat in DEGRIDDER_NAMES.items():
        assert idg_amd.kernel_name("degridder", S, 16,
                                   Options(degridder=impl)) \
            == pat.format(SUFFIX[S])
    # the gridder's option does not touch the degridder and vice versa
    assert idg_amd.kernel_name("degridder", S, 16, Options(gridder="auto")) \
        == DEGRIDDER_NAMES["default"].format(SUFFIX[S])
    # ... and the same names by environment, auto included
    for impl, pat in GRIDDER_NAMES.items():
        monkeypatch.setenv("IDG_GRIDDER_IMPL", impl)
        assert idg_amd.kernel_name("gridder", S, 16) == pat.format(SUFFIX[S])


def test_explicit_field_beats_contrary_variable(monkeypatch):
    monkeypatch.setenv("IDG_GRIDDER_IMPL", "sequential")
    monkeypatch.setenv("IDG_DEGRIDDER_IMPL", "sequential")
    assert idg_amd.kernel_name("gridder", 32, 16) == \
        "gridder_sequential_mi355x_s32"
    assert idg_amd.kernel_name("gridder", 32, 16, Options(gridder="default")) \
        == "gridder_mi355x_s32"
    assert idg_amd.kernel_name("gridder", 32, 16, Options(gridder="auto")) \
        == "gridder_auto_mi355x_s32"
    assert idg_amd.kernel_name("degridder", 32, 16,
                               Options(degridder="default")) == \
        "degridder_mi355x_s32"
    # the other direction: variable says default (or nothing), option wins
    monkeypatch.setenv("IDG_GRIDDER_IMPL", "default")
    monkeypatch.delenv("IDG_DEGRIDDER_IMPL")
    assert idg_amd.kernel_name("gridder", 64, 16,
                               Options(gridder="sequential")) == \
        "gridder_sequential_mi355x_s64"
    assert idg_amd.kernel_name("degridder", 64, 16,
                               Options(degridder="sequential")) == \
        "degridder_sequential_mi355x_s64"


def test_precision_by_option(monkeypatch):
    assert idg_amd.precision_options("gridder", 32, 256)[0] == 3
    # bits = 0 can be forced, against the default and against the variable
    assert idg_amd.precision_options("gridder", 32, 256,
                                     Options(precision=0))[0] == 0
    monkeypatch.setenv("IDG_PREC", "3")
    assert idg_amd.precision_options("gridder", 32, 256,
                                     Options(precision=0))[0] == 0
    assert idg_amd.precision_options("degridder", 32, 256,
                                     Options(precision=0))[0] == 0
    monkeypatch.setenv("IDG_PREC", "0")
    assert idg_amd.precision_options("gridder", 32, 256,
                                     Options(precision=3))[0] == 3
    assert idg_amd.precision_options("degridder", 32, 16,
                                     Options(precision=1))[0] == 1
    # each forced value is what IDG_PREC forces
    for bits in range(8):
        monkeypatch.setenv("IDG_PREC", str(bits))
        want = [idg_amd.precision_options(d, S, 256)[0]
                for d in ("gridder", "degridder") for S in SIZES]
        monkeypatch.setenv("IDG_PREC", str(bits ^ 7))
        got = [idg_amd.precision_options(d, S, 256,
                                         Options(precision=bits))[0]
               for d in ("gridder", "degridder") for S in SIZES]
        assert got == want, bits
    monkeypatch.delenv("IDG_PREC")
    # auto reports the MFMA pass's bits
    assert idg_amd.precision_options("gridder", 32, 256,
                                     Options(gridder="auto"))[0] == 3
    assert idg_amd.precision_options(
        "gridder", 32, 256, Options(gridder="auto", precision=1))[0] == 1
    assert idg_amd.precision_options("gridder", 32, 256,
                                     Options(gridder="ordered"))[0] == 0


def _invalid(make):
    o = _zero_struct()
    make(o)
    p = ctypes.cast(ctypes.pointer(o), ctypes.c_void_p)
    assert lib.idg_precision_options_opts(0, 32, 16, p) == E_INVALID
    msg = lib.idg_last_error().decode()
    assert "idg_options_t" in msg, msg
    assert lib.idg_kernel_name_opts(0, 32, 16, p) is None
    md = np.zeros(1, idg_amd.METADATA_DTYPE)
    assert lib.idg_auto_selected(1, 16, p, md.ctypes.data_as(ctypes.c_void_p),
                                 None) == E_INVALID
    # the launch entries refuse before they touch a buffer or the device
    assert lib.idg_gridder_launch_opts(
        1, 64, 32, 0.01, 0.0, 16, 2, None, None, None, None, None, None,
        None, None, p) == E_INVALID
    assert lib.idg_degridder_launch_opts(
        1, 64, 32, 0.01, 0.0, 16, 2, None, None, None, None, None, None,
        None, None, p) == E_INVALID
    assert lib.idg_gridder_fft_launch_opts(
        1, 64, 32, 0.01, 0.0, 16, 2, None, None, None, None, None, None,
        None, None, p) == E_INVALID
    assert lib.idg_c_run_gridder_opts(
        1, 64, 32, 0.01, 0.0, 16, 2, None, 0, None, None, None, None, 0,
        None, None, p) == E_INVALID
    assert lib.idg_c_run_degridder_opts(
        1, 64, 32, 0.01, 0.0, 16, 2, None, 0, None, None, None, None, 0,
        None, None, p) == E_INVALID
    return msg


@pytest.mark.parametrize("field,value", [
    ("gridder_impl", 6), ("gridder_impl", 0xffffffff),
    ("degridder_impl", 2),   # valu: by environment only
    ("degridder_impl", 4),   # ordered
    ("degridder_impl", 5),   # auto
    ("degridder_impl", 6),
    ("precision", 1), ("precision", 7), ("precision", 16), ("precision", 24),
    ("kernel_form", 3), ("fft_fusion", 3),
    ("struct_size", 0), ("struct_size", 2), ("struct_size", 6),
    ("struct_size", 27), ("struct_size", 1 << 20),
])
def test_invalid_options(field, value):
    msg = _invalid(lambda o: setattr(o, field, value))
    assert msg


def test_degridder_strings_ordered_and_auto_are_invalid():
    for impl in ("ordered", "auto", "valu"):
        with pytest.raises(idg_amd.IdgError) as e:
            idg_amd.kernel_name("degridder", 32, 16, Options(degridder=impl))
        assert e.value.code == E_INVALID
        assert "degridder_impl" in str(e.value)
    with pytest.raises(ValueError):
        Options(gridder="fastest").struct()


def test_larger_struct_size():
    class Newer(ctypes.Structure):
        _fields_ = [("known", OptionsStruct), ("later", ctypes.c_uint32 * 3)]
    n = Newer()
    n.known.struct_size = ctypes.sizeof(Newer)
    n.known.gridder_impl = 4
    p = ctypes.cast(ctypes.pointer(n), ctypes.c_void_p)
    # zero past the known fields: accepted, and the known fields count
    assert lib.idg_kernel_name_opts(0, 32, 16, p) == \
        b"gridder_ordered_mi355x_s32"
    for i in range(3):
        n.later[i] = 1
        assert lib.idg_kernel_name_opts(0, 32, 16, p) is None
        assert lib.idg_precision_options_opts(0, 32, 16, p) == E_INVALID
        assert "struct_size" in lib.idg_last_error().decode()
        n.later[i] = 0
    n.later[2] = 0x01000000     # the last byte alone
    assert lib.idg_precision_options_opts(0, 32, 16, p) == E_INVALID


def test_abi_version_is_still_1():
    assert idg_amd.abi_version() == 1


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "opts.c"
    src.write_text('#include "idg_mi355x.h"\n'
                   "idg_options_t o = {0};\n"
                   "int main(void) { o.struct_size = sizeof o; "
                   "o.gridder_impl = IDG_IMPL_AUTO; return (int)o.precision; }\n")
    r = subprocess.run(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror",
                        "-fsyntax-only", "-I", os.path.join(REPO, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(OptionsStruct) == 28


# -- auto_selected against numpy ---------------------------------------------
def _md(nr_timesteps):
    md = np.zeros(len(nr_timesteps), idg_amd.METADATA_DTYPE)
    md["nr_timesteps"] = nr_timesteps
    return md


def test_auto_selected_small_threshold():
    T = np.array([0, 3, 4, 5, 16] * 5 + [-1, -7], np.int32)
    md = _md(T)
    got = idg_amd.auto_selected(md, 16, Options(auto_threshold=64))
    want = ((T > 0) & (T.astype(np.int64) * 16 > 64)).astype(np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # exactly T x C > 64: T = 4 (= 64) is not, T = 5 is
    assert list(got[:5]) == [0, 0, 0, 1, 1]
    # a threshold above every product, and 1
    assert not idg_amd.auto_selected(md, 16, Options(auto_threshold=256)).any()
    assert np.array_equal(
        idg_amd.auto_selected(md, 16, Options(auto_threshold=1)),
        (T > 0).astype(np.uint8))
    # the threshold applies whatever gridder the options name
    assert np.array_equal(
        idg_amd.auto_selected(md, 16, Options(gridder="default",
                                              auto_threshold=64)), want)


def test_auto_selected_library_threshold():
    md = _md([64, 65, 128, 0, 63])
    assert idg_amd.api.AUTO_THRESHOLD == 16384
    for o in (None, Options(), Options(gridder="auto"), _zero_struct()):
        assert list(idg_amd.auto_selected(md, 256, o)) == [0, 1, 1, 0, 0]
    assert list(idg_amd.auto_selected(md, 257, None)) == [1, 1, 1, 0, 0]


def test_auto_selected_product_past_2_31():
    # 70,000 x 40,000 = 2.8e9 > 2^31: negative in 32 bits
    md = _md([70000, 2 ** 31 - 1, 1])
    assert list(idg_amd.auto_selected(md, 40000, None)) == [1, 1, 1]
    top = Options(auto_threshold=2 ** 32 - 1)
    assert list(idg_amd.auto_selected(md, 40000, top)) == [0, 1, 0]
    assert list(idg_amd.auto_selected(md, 2, top)) == [0, 0, 0]
    assert list(idg_amd.auto_selected(md, 3, top)) == [0, 1, 0]
    # a count only
    assert lib.idg_auto_selected(
        3, 40000, None, md.ctypes.data_as(ctypes.c_void_p), None) == 3
