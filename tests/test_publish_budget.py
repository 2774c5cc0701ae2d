"""Register / scratch / LDS budget of the published-policy kernels (csrc/kernels/k_publish.h), read from the built library's gfx950 code object (no GPU needed; after
tests/test_feedback_budget.py)."""
import os
import re
import subprocess
import tempfile

import pytest
import test_kernel_budgets as kb


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.READELF)), reason="libqmhip.so / llvm-readelf not available")
def test_published_policy_kernels_stay_in_registers():
    """qm_policy_publish_kernel: a copy of 464 sixteen-byte pieces per wavefront, eight in flight per lane — recorded at 38 registers, bound 64 (eight waves per SIMD);
    qm_policy_fb_pub_kernel: qm_policy_fb_kernel's body on another record view — recorded at the same 145 registers, bound: that kernel's count in the same build + 8.
    Neither has scratch or LDS"""
    k = kb._kernels()
    for name in ("qm_policy_publish_kernel", "qm_policy_fb_pub_kernel"):
        assert k[name]["scratch"] == 0 and k[name]["lds"] == 0, (name, k[name])
    assert k["qm_policy_publish_kernel"]["vgpr"] <= 64, k["qm_policy_publish_kernel"]
    assert k["qm_policy_fb_pub_kernel"]["vgpr"] <= k["qm_policy_fb_kernel"]["vgpr"] + 8, (k["qm_policy_fb_pub_kernel"], k["qm_policy_fb_kernel"])


@pytest.mark.skipif(not (os.path.exists(kb.LIB) and os.path.exists(kb.OBJDUMP)), reason="libqmhip.so / llvm-objdump not available")
def test_published_policy_kernels_have_no_barrier_and_stream_with_the_hint():
    """no s_barrier in either kernel; every global access of the publish kernel's record copy is a 16-byte one carrying `nt`"""
    body = {}
    for co in kb._code_objects():
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(co); f.flush(); dis = subprocess.run([kb.OBJDUMP, "-d", "--mcpu=gfx950", f.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <_Z\d+(qm_\w+_kernel)\w*>:", line)
            if m: cur = m.group(1); body.setdefault(cur, []); continue
            if cur: body[cur].append(line)
    for name in ("qm_policy_publish_kernel", "qm_policy_fb_pub_kernel"):
        assert name in body, sorted(body)
        assert not [l for l in body[name] if re.search(r"\bs_barrier\b", l)], name
    x4 = [l for l in body["qm_policy_publish_kernel"] if re.search(r"\bglobal_(load|store)_dwordx4\b", l)]
    assert len(x4) == 16 and all(re.search(r"\bnt\b", l) for l in x4), x4
