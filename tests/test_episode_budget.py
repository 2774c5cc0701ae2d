"""Resources of the episode monitor's kernels (csrc/kernels/k_episode.h), read from the built library's gfx950 code object (no GPU needed; after
tests/test_plan_budget.py)."""
import os
import re
import subprocess
import tempfile

import pytest

import test_kernel_budgets as kb

RECORDED = {"qm_episode_tick_kernel": 34, "qm_episode_mpc_kernel": 7}      # vector registers of the build this test was written against
GRANULE = 8


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.READELF)), reason="libqmhip.so / llvm-readelf not available")
def test_episode_kernels_use_no_scratch_no_lds_and_few_registers():
    """no private segment and no static LDS in either (their launches ask for no dynamic LDS); recorded register counts 34 / 7, the bound is the recorded value plus one
    allocation granule (8 registers), and 128: the wave-per-instance fold must never be what limits the occupancy of the WBC / plant kernels it runs between"""
    k = kb._kernels()
    for name, regs in RECORDED.items():
        assert name in k, sorted(n for n in k if n.startswith("qm_episode"))
        print(name, k[name])
        assert k[name]["scratch"] == 0 and k[name]["lds"] == 0, (name, k[name])
        assert k[name]["vgpr"] <= regs + GRANULE and k[name]["vgpr"] <= 128, (name, k[name])


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.OBJDUMP)), reason="libqmhip.so / llvm-objdump not available")
def test_episode_tick_kernel_has_no_barrier_and_no_atomics():
    """one wavefront per instance, reductions through DPP: no s_barrier, no atomics"""
    body = {}
    for co in kb._code_objects():
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(co); f.flush(); dis = subprocess.run([kb.OBJDUMP, "-d", "--mcpu=gfx950", f.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <_Z\d+(qm_\w+_kernel)\w*>:", line)
            if m: cur = m.group(1); body.setdefault(cur, []); continue
            if cur: body[cur].append(line)
    name = "qm_episode_tick_kernel"
    assert name in body and len(body[name]) > 50, sorted(body)
    assert not [l for l in body[name] if re.search(r"\bs_barrier\b|\bglobal_atomic|\bflat_atomic|\bds_(add|cmpst|max|min)_", l)], name
    assert [l for l in body[name] if "row_shr" in l or "row_bcast" in l], "the reductions are expected to be DPP steps"
