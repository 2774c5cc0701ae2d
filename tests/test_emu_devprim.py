"""The shared device primitives of qm_dev_common.h on the host emulator, one primitive per kernel (tests/devprim/devprim_kernels.h), against exact references
(tests/devprim_cases.py; the same cases run on gfx950 in tests/test_gpu_devprim.py).

The scalar maps run on FOUR builds: the emulator's exact stand-ins for v_rcp_f64 / v_rsq_f64, and estimates wrong by a relative 2^-EST_BITS with alternating, positive and
negative sign — the correction steps of qm_frcp, qm_log, qm_recip, qm_rsqrt, qm_rsqrt_n2, qm_givens, qm_house_scalars and the barrier derivatives must deliver their bounds
from the worst estimate the project claims, not from an exact reciprocal.  The structural checks (lane crossing, fragments, copies) do not depend on the estimates and run
on the exact build; what the emulator cannot express — the hardware's own DPP, MFMA and global-to-LDS semantics — is what the GPU test adds."""
import pytest
import devprim_cases as cases
import devprim_harness

_LIBS = {}


def _lib(label):
    if not _LIBS:
        _LIBS.update({p.label: p for p in devprim_harness.emu_libs(cases.EST_BITS)})
    return _LIBS[label]


@pytest.mark.parametrize("name", sorted(cases.SCALAR_CHECKS))
@pytest.mark.parametrize("label", ["emu", "emu_est_alt", "emu_est_plus", "emu_est_minus"])
def test_scalar_primitive(label, name):
    cases.SCALAR_CHECKS[name](_lib(label))


@pytest.mark.parametrize("name", sorted(cases.STRUCT_CHECKS))
def test_structural_primitive(name):
    cases.STRUCT_CHECKS[name](_lib("emu"))
