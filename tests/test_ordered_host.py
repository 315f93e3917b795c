"""The ordered gridder (IDG_GRIDDER_IMPL=ordered) on the host side: kernel
selection and reporting through the C ABI, and the design bound its GPU bars
rest on (tests/emul/ordered_emul.py).  No GPU needed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emul"))


@pytest.fixture(scope="module")
def idg():
    import idg_amd
    return idg_amd


def test_ordered_selection_and_reporting(idg, monkeypatch):
    before = idg.kernel_name("degridder", 32, 16)
    monkeypatch.setenv("IDG_GRIDDER_IMPL", "ordered")
    assert idg.kernel_name("gridder", 32, 16) == "gridder_ordered_mi355x_s32"
    assert idg.kernel_name("gridder", 64, 16) == "gridder_ordered_mi355x_s64"
    assert idg.kernel_name("gridder", 33, 16) == \
        "gridder_ordered_mi355x_generic"
    assert idg.precision_options("gridder", 32, 256)[0] == 0
    # IDG_GRIDDER_IMPL is the gridder's alone
    assert idg.kernel_name("degridder", 32, 16) == before
    monkeypatch.delenv("IDG_GRIDDER_IMPL")
    assert idg.kernel_name("gridder", 32, 16) == "gridder_mi355x_s32"


def test_ordered_emulation_design_bound_at_c256():
    """The reference's order with revolutions() and correctly rounded
    sin / cos (`rev`, deterministic), on the two -c subgrids at T x C =
    32,768: <= 2e-6 from the oracle (measured 1.18e-6 and 1.24e-6).  What is
    left of the GPU test's 5e-6 is the hardware sin / cos' to spend."""
    from ordered_emul import distances
    d = distances(128, 256, "rev", subgrids=(0, 1))
    print("ordered_emul rev, T x C = 128 x 256:", ["%.3e" % x for x in d])
    assert max(d) <= 2e-6, d
