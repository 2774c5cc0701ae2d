"""Resources of the two kernels of the streamed controller tick (csrc/kernels/k_tick.h), read from the built library's gfx950 code object (no GPU needed; after
tests/test_feedback_budget.py)."""
import os

import pytest

import test_kernel_budgets as kb

RECORDED = {"qm_tick_state_kernel": 18, "qm_tick_pack_kernel": 20}      # vector registers of the build this test was written against
GRANULE = 8


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.READELF)), reason="libqmhip.so / llvm-readelf not available")
def test_tick_kernels_use_no_scratch_no_lds_and_few_registers():
    """qm_tick_state_kernel (one thread per instance: unwrapping, safety, measured mode) and qm_tick_pack_kernel (one workgroup per instance: control law + record) are
    glue: no private segment, no LDS.  Recorded register counts: 18 and 20; the bound is the recorded value plus one allocation granule (8 registers)"""
    k = kb._kernels()
    for name, regs in RECORDED.items():
        assert name in k, sorted(n for n in k if n.startswith("qm_tick"))
        print(name, k[name])
        assert k[name]["scratch"] == 0 and k[name]["lds"] == 0, (name, k[name])
        assert k[name]["vgpr"] <= regs + GRANULE, (name, k[name])
