"""Resources of the two instances of the plant kernel (csrc/kernels/k_sim.h), read from the built library's gfx950 code object (no GPU needed; after
tests/test_episode_budget.py)."""
import os

import pytest

import test_kernel_budgets as kb

PUSH_RECORDED = 414      # vector registers (arch + acc) of qm_sim_push_kernel in the build this test was written against
GRANULE = 8
PLAIN = dict(vgpr=392, scratch=0, lds=0)      # qm_sim_kernel as the commit before the push kernel built it: the template's `false` instance must stay what it was


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.READELF)), reason="libqmhip.so / llvm-readelf not available")
def test_push_kernel_uses_no_scratch_no_static_lds_and_the_plain_kernel_is_unchanged():
    """the push instance: one wavefront per instance in the plain kernel's dynamic LDS carve (SIM_LDS_BYTES), no private segment, recorded 414 registers with one allocation
    granule of room; the plain instance: exactly the registers, scratch and static LDS it had before the body moved into the template"""
    k = kb._kernels()
    assert "qm_sim_push_kernel" in k and "qm_sim_kernel" in k, sorted(n for n in k if n.startswith("qm_sim"))
    print("qm_sim_push_kernel", k["qm_sim_push_kernel"], "qm_sim_kernel", k["qm_sim_kernel"])
    assert k["qm_sim_push_kernel"]["scratch"] == 0 and k["qm_sim_push_kernel"]["lds"] == 0, k["qm_sim_push_kernel"]
    assert k["qm_sim_push_kernel"]["vgpr"] <= PUSH_RECORDED + GRANULE, k["qm_sim_push_kernel"]
    assert k["qm_sim_kernel"] == PLAIN, k["qm_sim_kernel"]
