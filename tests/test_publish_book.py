"""The slot / sequence / mutex bookkeeping of the published policy (csrc/host/qm_publish_book.h) in a stand-alone host program with a stub device
(tests/pub_book/pub_book_main.cpp), built with the address + undefined-behaviour sanitizers and with the thread sanitizer and run directly.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "pub_book", "pub_book_main.cpp")


@pytest.mark.parametrize("name,flags", [("asan_ubsan", "-fsanitize=address,undefined"), ("tsan", "-fsanitize=thread")])
def test_publication_bookkeeping_under_sanitizers(name, flags):
    """one publisher, three evaluators, 2000 publications: no evaluation ever sees a slot that is being filled (no data race, no torn stamp), the sequence number never goes
    back, a publication waits for a slot's evaluation event exactly when one was recorded since the slot was last filled, and nothing is handed out without a window"""
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    bdir = os.path.join(ROOT, "tests", "_build"); os.makedirs(bdir, exist_ok=True); exe = os.path.join(bdir, "pub_book_" + name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", flags, SRC, "-lpthread", "-o", exe])
    p = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "result ok" in p.stdout, p.stdout + p.stderr
    assert "Sanitizer" not in p.stderr, p.stderr
