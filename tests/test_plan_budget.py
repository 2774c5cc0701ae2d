"""Resources of the three task-space plan kernels (csrc/kernels/k_plan.h), read from the built library's gfx950 code object (no GPU needed; after
tests/test_tick_budget.py)."""
import os
import re
import subprocess
import tempfile

import pytest

import plan_ref as pf
import test_kernel_budgets as kb

RECORDED = {"qm_plan_nodes_kernel": 208, "qm_plan_states_kernel": 208, "qm_plan_footholds_kernel": 128}      # vector registers of the build this test was written against
GRANULE = 8


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.READELF)), reason="libqmhip.so / llvm-readelf not available")
def test_plan_kernels_use_no_scratch_and_stay_in_their_registers():
    """no private segment in any of the three; recorded register counts 208 / 208 / 128, the bound is the recorded value plus one allocation granule (8 registers) — and
    for the row kernels 256, two waves per SIMD as for K1a.  The two row kernels are one routine: the same count.  Their LDS is dynamic (the code object holds none):
    the launch's QM_PLAN_LDS_BYTES must let two waves per SIMD fit a CU's 160 KB beside each other, <= 24 KB"""
    k = kb._kernels()
    for name, regs in RECORDED.items():
        assert name in k, sorted(n for n in k if n.startswith("qm_plan"))
        print(name, k[name])
        assert k[name]["scratch"] == 0 and k[name]["lds"] == 0, (name, k[name])
        assert k[name]["vgpr"] <= regs + GRANULE, (name, k[name])
    assert k["qm_plan_nodes_kernel"]["vgpr"] == k["qm_plan_states_kernel"]["vgpr"] <= 256
    lds = pf.emu_lib().emu_plan_layout(15); assert 0 < lds <= 24 * 1024 and 8 * lds <= 160 * 1024, lds


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.OBJDUMP)), reason="libqmhip.so / llvm-objdump not available")
def test_plan_kernels_have_no_barrier_and_no_atomics():
    """wave-level ordering only (no s_barrier) and a computed slot order (no atomics) in the three kernels"""
    body = {}
    for co in kb._code_objects():
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(co); f.flush(); dis = subprocess.run([kb.OBJDUMP, "-d", "--mcpu=gfx950", f.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <_Z\d+(qm_\w+_kernel)\w*>:", line)
            if m: cur = m.group(1); body.setdefault(cur, []); continue
            if cur: body[cur].append(line)
    for name in RECORDED:
        assert name in body, sorted(body)
        assert not [l for l in body[name] if re.search(r"\bs_barrier\b|\bglobal_atomic|\bflat_atomic|\bds_(add|cmpst|max|min)_", l)], name
