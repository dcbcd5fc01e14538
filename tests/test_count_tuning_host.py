"""The count stage's environment knobs (reflexiv_amd/csrc/rfx_count_tuning.h: count_tuning, sweep_level1, wide_records_enabled)
as HOST code: tests/count_tuning_main.cpp, compiled with the host compiler under -fsanitize=address,undefined and run as a child
process.  It pins every default, the parsing quirks the GPU tests rely on, and that nothing is cached between calls.
Needs no GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reflexiv_amd", "csrc")


def test_count_knobs_parse_as_they_always_did_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    assert os.path.exists(os.path.join(CSRC, "rfx_count_tuning.h"))
    exe = str(tmp_path / "count_tuning")
    # (the sanitizer runtimes linked into the program itself: it depends on no load order)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or os.path.basename(cxx) == "c++" else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I" + CSRC,
                    os.path.join(HERE, "count_tuning_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    # (a clean environment for the child apart from what it sets itself)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RFX_")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout


def test_getenv_stays_in_the_tuning_header():
    """the count stage's sources read the environment only through rfx_count_tuning.h"""
    names = ["rfx_kmer.hip", "rfx_synth.hip", "rfx_count.h"] + sorted(
        f for f in os.listdir(CSRC) if f.startswith("rfx_count_") and f.endswith(".hip"))
    assert "rfx_count_sk.hip" in names
    for name in names:
        assert "getenv" not in open(os.path.join(CSRC, name)).read(), name
