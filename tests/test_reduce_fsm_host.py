"""The per-row transition of the reduction stage's two window adjustments (reflexiv_amd/csrc/rfx_reduce_fsm.h) as HOST code:
tests/reduce_fsm_main.cpp runs the reference's sequential two-pending-row loop, written directly, against the map / scan / emit
formulation the kernels use, over every sequence of up to 7 rows of a small alphabet and seeded random sequences of 10,000 rows cut
into partitions.  Compiled with the host compiler under -fsanitize=address,undefined and run as a child process.  Needs no GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reflexiv_amd", "csrc")


def test_scan_formulation_equals_the_sequential_loop_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    assert os.path.exists(os.path.join(CSRC, "rfx_reduce_fsm.h"))
    exe = str(tmp_path / "reduce_fsm")
    # (the sanitizer runtimes linked into the program itself: it depends on no load order)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or os.path.basename(cxx) == "c++" else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I" + CSRC,
                    os.path.join(HERE, "reduce_fsm_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
