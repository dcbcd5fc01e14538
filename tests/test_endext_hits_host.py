"""eh_row and eh_add (reflexiv_amd/csrc/rfx_endext_hits.h) -- what rfx_dev_endext_consensus_hits computes from a hit of the end mapping
in place of printing a row and parsing it back -- as HOST code against the two string models: tests/endext_hits_main.cpp, compiled with
the host compiler under -fsanitize=address,undefined and run as a child process, writes the row and the contributions of every hit
of its enumeration (reads of 22..340 bases, every offset, both sides, whole-contig and 200-base targets; v at both of its limits);
here the same enumeration goes through map_model.row_of and endext_model.contributions.  Needs no GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import endext_model as E
from tests import map_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reflexiv_amd", "csrc")
SEED = 21
TARGETS = (60, 399, 400)


def model_hits():
    """every placement the mapper's definition allows, in the host program's order: target, read length, side, offset -> (side, L, n,
    off, v, p, overhang, name, target length)"""
    for L in TARGETS:
        whole = L < 2 * M.END
        tlen = L if whole else M.END
        ident = f"Contig_{L}_-1_2_0"
        for n in range(SEED + 1, 341):
            for side in (0, 1):
                name = ident + ("" if whole else ("-L", "-R")[side])
                if side == 0:
                    for off in range(1, n - SEED + 1):
                        v = min(n - off, tlen)
                        yield side, L, n, off, v, n - off - v, off, name, tlen
                else:
                    for off in range(0, n - 1 - SEED + 1):
                        v = min(off + SEED, tlen)
                        yield side, L, n, off, v, off + SEED - v, n - off - SEED, name, tlen


def test_rows_and_contributions_of_every_hit_equal_the_models_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe, out = str(tmp_path / "endext_hits"), str(tmp_path / "hits.bin")
    # (the sanitizer runtimes linked into the program itself: it depends on no load order)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or os.path.basename(cxx) == "c++" else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I" + CSRC,
                    os.path.join(HERE, "endext_hits_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.fromfile(out, np.int32).reshape(-1, 16).tolist()
    assert r.stdout.split() == ["ok", str(len(got))]
    rng = np.random.default_rng(33)
    reads = {n: M.rand_seq(rng, n) for n in range(SEED + 1, 341)}
    seen = {"v = rest": 0, "v = target": 0, "left": 0, "right": 0, "both": 0, "one base": 0, "cut": 0}
    k = 0
    for side, L, n, off, v, p, over, name, tlen in model_hits():
        g = got[k]
        k += 1
        assert g[:5] == [side, L, n, off, v], (k, g)
        seq = reads[n]
        row = M.row_of((0, side, 0, off, v, p, over, name, seq, tlen))
        suf, start, c0, c1, c2, lsrc, lcnt, rsrc, rcnt, bad = g[5:15]
        cigar = (f"{c0}S" if c0 else "") + f"{c1}M" + (f"{c2}S" if c2 else "")
        want_name = f"Contig_{L}_-1_2_0" + ("", "-L", "-R")[suf]
        assert row == f"{want_name}\t{start}\t{cigar}\t{seq}", (g, row)
        left, right = E.contributions(*row.split("\t"))
        assert bad == 0 and lcnt == min(len(left), E.LONGEST) and rcnt == min(len(right), E.LONGEST), (g, len(left), len(right))
        if lcnt:
            assert lsrc == len(left) - 1 and left[:lcnt] == seq[lsrc - lcnt + 1:lsrc + 1][::-1], g
        if rcnt:
            assert rsrc == n - len(right) and right[:rcnt] == seq[rsrc:rsrc + rcnt], g
        seen["v = rest" if v < tlen else "v = target"] += 1
        seen["left"] += bool(lcnt)
        seen["right"] += bool(rcnt)
        seen["both"] += bool(lcnt and rcnt)
        seen["one base"] += side == 0 and off == 1 and not lcnt
        seen["cut"] += max(len(left), len(right)) > E.LONGEST
    assert k == len(got)
    assert all(seen.values()), seen
