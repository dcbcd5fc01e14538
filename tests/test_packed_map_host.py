"""pk_mismatch32 and pk_rc_seg32 (reflexiv_amd/csrc/rfx_packed_words.h), the word helpers the end mapping adds, as HOST code against
values written out by hand and a naive loop over bases: tests/packed_map_main.cpp, compiled with the host compiler under
-fsanitize=address,undefined and run as a child process.  Needs no GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reflexiv_amd", "csrc")


def test_the_mapping_word_helpers_equal_the_loop_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "packed_map")
    # (the sanitizer runtimes linked into the program itself: it depends on no load order)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or os.path.basename(cxx) == "c++" else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I" + CSRC,
                    os.path.join(HERE, "packed_map_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
