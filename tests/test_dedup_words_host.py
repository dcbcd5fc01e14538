"""The word helpers of the contig de-duplication (reflexiv_amd/csrc/rfx_dedup_words.h: dd_seg32, dd_seg32_rc, dd_cat32, the marker
31-mer, the 15-mer seed with its past-the-end rule) as HOST code against a byte model: tests/dedup_words_main.cpp, compiled with
the host compiler under -fsanitize=address,undefined and run as a child process.  Needs no GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reflexiv_amd", "csrc")


def test_word_helpers_equal_the_byte_model_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    assert os.path.exists(os.path.join(CSRC, "rfx_dedup_words.h"))
    exe = str(tmp_path / "dedup_words")
    # (the sanitizer runtimes linked into the program itself: it depends on no load order)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or os.path.basename(cxx) == "c++" else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I" + CSRC,
                    os.path.join(HERE, "dedup_words_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
