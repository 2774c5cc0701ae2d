"""Resources of the plant kernel's two terrain instances and of the lookup kernel (csrc/kernels/k_sim.h), read from the built library's gfx950 code object (no GPU needed;
after tests/test_push_budget.py), and of the two instances that were there before."""
import os

import pytest

import test_kernel_budgets as kb
import test_push_budget as pb

TERRAIN_RECORDED = 424           # vector registers (arch + acc) of qm_sim_terrain_kernel in the build this test was written against
TERRAIN_PUSH_RECORDED = 452      # ... of qm_sim_terrain_push_kernel
EVAL_RECORDED = 46               # ... of qm_terrain_eval_kernel
GRANULE = 8


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.READELF)), reason="libqmhip.so / llvm-readelf not available")
def test_terrain_kernels_use_no_scratch_no_static_lds_and_the_other_plant_kernels_are_unchanged():
    """the terrain instances: one wavefront per instance in the plain kernel's dynamic LDS carve (SIM_LDS_BYTES; the corner exchange lives in the accumulators' slots), no
    private segment, the recorded registers with one allocation granule of room; qm_terrain_eval_kernel likewise.  The plain instance: exactly what
    tests/test_push_budget.py records; the push instance: within its recorded bound"""
    k = kb._kernels(); new = {"qm_sim_terrain_kernel": TERRAIN_RECORDED, "qm_sim_terrain_push_kernel": TERRAIN_PUSH_RECORDED, "qm_terrain_eval_kernel": EVAL_RECORDED}
    assert all(n in k for n in new) and "qm_sim_kernel" in k and "qm_sim_push_kernel" in k, sorted(n for n in k if n.startswith("qm_sim") or n.startswith("qm_terrain"))
    for n, recorded in new.items():
        print(n, k[n])
        assert k[n]["scratch"] == 0 and k[n]["lds"] == 0 and k[n]["vgpr"] <= recorded + GRANULE, (n, k[n])
    assert k["qm_sim_kernel"] == pb.PLAIN, k["qm_sim_kernel"]
    assert k["qm_sim_push_kernel"]["scratch"] == 0 and k["qm_sim_push_kernel"]["lds"] == 0 and k["qm_sim_push_kernel"]["vgpr"] <= pb.PUSH_RECORDED + pb.GRANULE, k["qm_sim_push_kernel"]
