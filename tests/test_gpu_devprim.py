"""The shared device primitives of qm_dev_common.h on gfx950, one primitive per kernel (tests/devprim/devprim_kernels.h, built with the product's compiler flags into
tests/_build/libqm_devprim.so), against the exact references of tests/devprim_cases.py — the cases tests/test_emu_devprim.py runs on the host emulator.  Here the
hardware's own v_rcp_f64 / v_rsq_f64, DPP controls, v_readlane, v_mfma_f64_16x16x4_f64 fragment map and global-to-LDS copy are what is compared, not a stand-in
written from the project's reading of them.  A missing library that cannot be built is an error, not a skip."""
import json
import os
import pytest
import devprim_cases as cases
import devprim_harness

pytestmark = pytest.mark.gpu
_LIB = []


def _lib():
    if not _LIB:
        _LIB.append(devprim_harness.device_lib())
    return _LIB[0]


def test_raw_estimates_are_no_worse_than_the_modelled_ones():
    """v_rcp_f64 / v_rsq_f64: maximum relative error <= 2^-EST_BITS, the error tests/test_emu_devprim.py feeds the correction steps; the measurement goes to
    tests/_build/devprim_estimates.json (a copy of a device run belongs in profiles/devprim_estimates.json)"""
    try:
        cases.check_raw_estimates(_lib())
    finally:
        if cases.ESTIMATES:
            with open(os.path.join(os.path.dirname(devprim_harness.DEVICE_LIB), "devprim_estimates.json"), "w") as f:
                json.dump({"est_bits_asserted": cases.EST_BITS, **cases.ESTIMATES}, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("name", sorted(set(cases.SCALAR_CHECKS) - {"raw_estimates"}))
def test_scalar_primitive(name):
    cases.SCALAR_CHECKS[name](_lib())


@pytest.mark.parametrize("name", sorted(cases.STRUCT_CHECKS))
def test_structural_primitive(name):
    cases.STRUCT_CHECKS[name](_lib())
