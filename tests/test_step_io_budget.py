"""Resources of the step-I/O pack kernel, read from the built library's gfx950 code object (no GPU needed): a plain bandwidth kernel — no private segment, no LDS."""
import os

import pytest

import test_kernel_budgets as kb


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.READELF)), reason="libqmhip.so / llvm-readelf not available")
def test_pack_kernel_uses_no_scratch_and_no_lds():
    k = kb._kernels()
    assert "qm_step_pack_kernel" in k, sorted(n for n in k if n.startswith("qm_"))
    assert k["qm_step_pack_kernel"]["scratch"] == 0 and k["qm_step_pack_kernel"]["lds"] == 0, k["qm_step_pack_kernel"]
    assert k["qm_step_pack_kernel"]["vgpr"] <= 64, k["qm_step_pack_kernel"]      # eight waves per SIMD: latency hiding is all a copy kernel has
