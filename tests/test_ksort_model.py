"""The k-mer sorting stage without a GPU: the string model (tests/ksort_model.py) equals every stage of every case the reference's
own classes made (tests/golden/ksort_vectors.npz), the vectors regenerate byte for byte, the header declares the entry points and
_lib binds them, and reflexiv_host knows `sort`."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import ksort_model as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "ksort_vectors.npz")
REF = os.environ.get("RFX_REFERENCE", "/root/reference")
SYMBOLS = ["rfx_ksort_default_params", "rfx_dev_ksort_binarize", "rfx_dev_ksort_fork_filter", "rfx_dev_ksort_reflect",
           "rfx_dev_ksort_full_kmers", "rfx_dev_ksort_to_text", "rfx_dev_ksort_run", "rfx_ksort_text"]
ALL_K = (8, 23, 31, 33, 34, 62, 64, 65, 66, 95, 96, 97, 98, 124)


def names():
    return [str(x) for x in np.load(VEC)["names"]]


def test_the_cases_are_the_ones_the_stage_is_pinned_on():
    z = np.load(VEC)
    got = {n: K.load_case(z, n)[0] for n in names()}
    for k in ALL_K:
        for mk in {k, 97}:
            assert got[f"k{k}_m{mk}"] == K.default_params(k, max_k=mk)
    assert got["k31_E4_F2"]["min_error_cov"] == 4 and got["k31_E4_F2"]["min_repeat_fold"] == 2.0
    assert got["k31_maxcov12"]["max_cov"] == 12 and got["k33_bubble0"]["bubble"] == 0
    assert os.path.getsize(VEC) < (1 << 20)
    # what the reference's classes do at the refused k: rows [k, input rows, output rows, output rows that are no input k-mer]: nothing comes out, or rows that were never put in
    r = z["refused_k"]
    assert r[:, 0].tolist() == [32, 63, 94] and all(not K.supported_k(int(k)) for k in r[:, 0])
    assert all(int(out) == 0 or int(bad) > 0 for _, _, out, bad in r), r.tolist()


@pytest.mark.parametrize("case", names())
def test_the_model_equals_every_stage_of_the_reference(case):
    p, rows, st, text = K.load_case(np.load(VEC), case)
    got = K.run_stages(rows, p)
    assert sorted(got) == sorted(st)
    for s in K.STAGES:
        if s in st:
            assert got[s] == st[s], (case, s, next(i for i, (a, b) in enumerate(zip(got[s] + [None], st[s] + [None])) if a != b))
    assert K.to_text(got["s8"], p["k"]) == text
    if p["bubble"]:
        M = p["max_k"] + 3
        assert {v for r in st["s8"] for v in r[3:]} <= {-1, M}          # the counts themselves do not survive the stage
    assert K.handover(text) == [(r[0][:-1], r[0][-1], 1, r[3], r[4]) for r in st["s8"]]


def test_the_crafted_rows_are_in_the_cases():
    z = np.load(VEC)
    p, rows, st, text = K.load_case(z, "k64_m64")
    assert any(r.startswith("(") and r.endswith(")\n") for r in rows) and any(r.endswith(",1234567890\n") for r in rows)
    assert any("N" in r for r in rows) and any(r.split(",")[0].islower() for r in rows)
    assert any(len(r.split(",")[0]) == 67 for r in rows)
    kmers = [r.split(",")[0] for r in rows]
    rc = lambda s: s.translate(K.COMP)[::-1]
    assert any(s == rc(s) for s in kmers) and any(rc(s) in kmers and rc(s) != s for s in kmers)
    p, rows, st, text = K.load_case(z, "k41_longrun")
    from collections import Counter
    assert max(Counter(r.split(",")[0] for r in rows).values()) == 600 and 900 <= len(rows) <= 1000


def test_the_vectors_regenerate_byte_for_byte(tmp_path):
    if not os.path.isdir(os.path.join(REF, "src", "main", "java")):
        pytest.skip("the reference's sources are not here")
    out = tmp_path / "ksort_vectors.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_ksort_vectors.py"), "--out", str(out), "--jobs", "8"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert out.read_bytes() == open(VEC, "rb").read()


def test_the_header_declares_the_entry_points_and_the_bindings_hold_them():
    from reflexiv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "reflexiv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS, name
    assert "rfx_ksort_params" in code
    assert [f for f, _ in _lib.CKsortParams._fields_] == ["k", "max_k", "min_error_cov", "max_cov", "bubble", "min_repeat_fold"]
    L = _lib.lib()
    p = _lib.CKsortParams()
    L.rfx_ksort_default_params(p, 41)
    assert (p.k, p.max_k, p.min_error_cov, p.max_cov, p.bubble, p.min_repeat_fold) == (41, 95, 8, 10000000, 1, 1.5)
    src = open(os.path.join(ROOT, "reflexiv_amd", "csrc", "rfx_ksort.hip")).read()
    assert "rfx_ksort.hip" in open(os.path.join(ROOT, "reflexiv_amd", "csrc", "Makefile")).read()
    for name in SYMBOLS[1:]:
        body = src[src.index("int %s(" % name):]
        body = body[:body.index("RFX_API_CATCH")]
        assert "hipSetDevice(ctx->device)" in body and "hipDeviceSynchronize" not in body, name


def test_reflexiv_host_knows_sort():
    from reflexiv_amd import _lib
    _lib.build()
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    assert os.path.exists(exe)
    r = subprocess.run([exe, "sort"], capture_output=True, text=True)
    assert r.returncode != 0 and "-kmerc" in r.stderr + r.stdout and "-kmer" in r.stderr + r.stdout
    r = subprocess.run([exe, "sort", "-kmerc", "x.csv", "-kmer", "32", "-outfile", "/nonexistent"], capture_output=True, text=True)
    assert r.returncode != 0 and "32" in r.stderr + r.stdout
