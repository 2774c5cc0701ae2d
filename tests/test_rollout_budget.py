"""Resources of the policy rollout kernel (qm_policy_rollout_kernel, csrc/kernels/k_rollout.h), read from the built library's gfx950 code object (kernel metadata only; no
GPU needed; after tests/test_plan_budget.py)."""
import os

import pytest

import test_kernel_budgets as kb

KERNEL = "qm_policy_rollout_kernel"
RECORDED = 256      # vector registers of both instances (stage records, published records) in the build this test was written against
GRANULE = 8


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.READELF)), reason="libqmhip.so / llvm-readelf not available")
def test_rollout_kernel_fits_two_waves_per_simd_without_a_private_segment():
    """every instance of the kernel — one body, two gain views — has no private segment, at most 256 vector registers (two waves per SIMD), and at most the count of the
    build this test was written against plus one allocation granule of 8.  (With the shared ilqr_rk2_lane the kernel took 266 / 268 registers, or 28 bytes of scratch
    under the cap: hence the restated step qm_ro_rk2_lane, k_rollout.h.)  Its LDS is the 1 KB the fold registers are parked in"""
    k = kb._kernels(); inst = {n: v for n, v in k.items() if KERNEL in n and n != KERNEL}
    assert len(inst) == 2, sorted(inst)
    for name, v in inst.items():
        print(name, v)
        assert v["scratch"] == 0, (name, v)
        assert v["vgpr"] <= 256, (name, v)
        assert v["vgpr"] <= RECORDED + GRANULE, (name, v)
        assert v["lds"] <= 1024, (name, v)
