"""Resources of the sensor kernel (csrc/kernels/k_sense.h) and of the two plant kernels it runs behind, read from the built library's gfx950 code object (no GPU needed;
after tests/test_push_budget.py)."""
import os

import pytest

import test_kernel_budgets as kb
import test_push_budget as pb

SENSE_RECORDED = 112      # vector registers (arch + acc) of qm_sense_kernel in the build this test was written against
GRANULE = 8


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.READELF)), reason="libqmhip.so / llvm-readelf not available")
def test_sense_kernel_uses_no_scratch_no_static_lds_and_the_plant_kernels_are_unchanged():
    """qm_sense_kernel: one wavefront per instance in a dynamic LDS carve (SENSE_LDS_BYTES; k_sense.h declares no static LDS), no private segment — the arm chain's per-joint
    composites live in LDS for that —, recorded 112 registers with one allocation granule of room.  The plant kernels: what tests/test_push_budget.py expects"""
    k = kb._kernels()
    assert "qm_sense_kernel" in k, sorted(n for n in k if n.startswith("qm_s"))
    print("qm_sense_kernel", k["qm_sense_kernel"], "qm_sim_push_kernel", k["qm_sim_push_kernel"], "qm_sim_kernel", k["qm_sim_kernel"])
    assert k["qm_sense_kernel"]["scratch"] == 0 and k["qm_sense_kernel"]["lds"] == 0, k["qm_sense_kernel"]
    assert k["qm_sense_kernel"]["vgpr"] <= SENSE_RECORDED + GRANULE, k["qm_sense_kernel"]
    assert k["qm_sim_kernel"] == pb.PLAIN, k["qm_sim_kernel"]
    assert k["qm_sim_push_kernel"]["scratch"] == 0 and k["qm_sim_push_kernel"]["lds"] == 0 and k["qm_sim_push_kernel"]["vgpr"] <= pb.PUSH_RECORDED + pb.GRANULE, k["qm_sim_push_kernel"]
