"""Register / scratch budget of the feedback-policy kernels, read from the built library's gfx950 code object (no GPU needed; after tests/test_kernel_budgets.py)."""
import os
import pytest
import test_kernel_budgets as kb


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.READELF)), reason="libqmhip.so / llvm-readelf not available")
def test_feedback_kernels_stay_in_registers():
    """qm_policy_fb_kernel is one wavefront per instance holding one row of K and one of Px per lane (60 doubles): recorded at 145 registers, no scratch, no LDS — three waves per
    SIMD; the bound leaves one allocation granule.  qm_feedback_gather_kernel: 24 registers.  Neither may touch the private segment"""
    k = kb._kernels()
    for name in ("qm_policy_fb_kernel", "qm_feedback_gather_kernel"):
        assert k[name]["scratch"] == 0 and k[name]["lds"] == 0, (name, k[name])
    assert k["qm_policy_fb_kernel"]["vgpr"] <= 160 and k["qm_feedback_gather_kernel"]["vgpr"] <= 64, (k["qm_policy_fb_kernel"], k["qm_feedback_gather_kernel"])
