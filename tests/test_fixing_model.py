"""The contig fixing stage without a GPU: the string model (tests/fixing_model.py) equals every stage of every case the
reference's own classes made (tests/golden/fixing_vectors.npz), every branch of both folds and of the loop is taken by the
cases, the folds' closed form holds, the vectors regenerate byte for byte, and the header declares the entry points that
_lib binds."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import fixing_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "fixing_vectors.npz")
REF = os.environ.get("RFX_REFERENCE", "/root/reference")
SYMBOLS = ["rfx_fix_default_params", "rfx_dev_fix_binarize", "rfx_dev_fix_contig_ends", "rfx_dev_fix_kmer_set", "rfx_dev_fix_fork_filter",
           "rfx_dev_fix_reflect", "rfx_dev_fix_run", "rfx_fix_text"]


def names():
    return [str(x) for x in np.load(VEC)["names"]]


@pytest.fixture(scope="module")
def cases():
    z = np.load(VEC)
    return {n: F.load_case(z, n) for n in names()}


def test_the_cases_are_the_ones_the_stage_is_pinned_on(cases):
    ps = [(c[0], c[1]) for c in cases.values()]
    assert {p["max_k"] for p, _ in ps} == {31, 32, 41, 99}
    assert {P for _, P in ps} == {1, 2, 7, 63}
    assert {p["scramble"] for p, _ in ps} == {2, 3}
    assert {p["max_iteration"] for p, _ in ps} == {0, 3, 150}
    assert os.path.getsize(VEC) < (1 << 20)
    for p, P, rows, st, sps, kmers, passes, text in cases.values():
        assert len(passes) == 1 + min(p["max_iteration"] + 1, 17)
    # 63 partitions of a few rows: empty ones, going in and coming out of both folds
    assert any(P == 63 and any(a == b for a, b in zip(sps[s], sps[s][1:])) for p, P, rows, st, sps, *_ in cases.values() for s in sps)


def test_every_branch_of_both_folds_and_of_the_loop_is_taken(cases):
    z = np.load(VEC)
    want = [f"{t} {b}" for t in "LR" for b in F.FOLD_BRANCHES if (t, b) != ("L", "short_after_long_dropped")] + list(F.LOOP_BRANCHES)
    assert [str(b) for b in z["branch_names"]] == want
    assert all(int(h) > 0 for h in z["branch_hits"]), dict(zip(z["branch_names"], z["branch_hits"]))
    hits = {}
    for p, P, rows, *_ in cases.values():
        F.run_stages(rows, p, P, hits)
    assert [hits.get(b, 0) for b in want] == [int(h) for h in z["branch_hits"]]
    assert "L short_after_long_dropped" not in hits               # (the union puts the 31-mer records first and the sort is stable)


@pytest.mark.parametrize("case", names())
def test_the_model_equals_every_stage_of_the_reference(cases, case):
    p, P, rows, st, ps, kmers, passes, text = cases[case]
    got, gps, gk, gpasses = F.run_stages(rows, p, P)
    assert gk == kmers
    for s in F.STAGES:
        assert got[s] == st[s], (case, s, next(i for i, (a, b) in enumerate(zip(got[s] + [None], st[s] + [None])) if a != b))
    assert gps == ps and all(len(v) == P + 1 for v in ps.values())
    assert len(gpasses) == len(passes)
    for i, (a, b) in enumerate(zip(gpasses, passes)):             # step 9 is the dynamic-k pass (pymodel.dyn_extend_pass), unchanged
        assert a == b, (case, "pass", i)
    assert F.to_text(gpasses[-1]) == text and F.run_text(rows, p, P) == text
    # capacities: contig ends from n alone, everything behind it bounded by its input
    n = len(st["binarized"])
    assert len(kmers) <= 2 * n * (p["max_k"] - 30) and len(st["long"]) <= n and len(st["union"]) <= len(kmers) + len(st["long"])
    assert len(st["fold1"]) <= len(st["sort1"]) and len(st["fold2"]) <= len(st["sort2"])
    assert all(len(b) <= len(a) for a, b in zip([st["fold2"]] + passes, passes))
    assert all(len(r[0]) == 30 for s in F.STAGES[1:] for r in st[s]) and all(len(r[0]) == 30 for q in passes for r in q)


@pytest.mark.parametrize("case", names())
def test_the_closed_form_of_the_folds_and_the_order_of_the_distinct_set(cases, case):
    p, P, rows, st, ps, kmers, passes, text = cases[case]
    for a, b in (("sort1", "fold1"), ("sort2", "fold2")):
        for q in range(P):
            assert F.fold_closed_form(st[a][ps[a][q]:ps[a][q + 1]]) == st[b][ps[b][q]:ps[b][q + 1]], (case, b, q)
    # the distinct 31-mers in the device's order (ascending) instead of first occurrence: the same from the first fold on
    got, gps, _, gpasses = F.run_stages(rows, p, P, order="sorted")
    assert got["union"] != st["union"] or len(set(kmers)) < 2
    assert all(got[s] == st[s] for s in ("fold1", "reflected", "sort2", "fold2")) and gps["fold1"] == ps["fold1"] and gpasses == passes


def test_the_fold_on_inputs_the_driver_never_makes():
    """a one-base row behind a longer row of its key (the left fold never sees it), ties of the smallest base, runs that mix"""
    K = "ACGT" * 7 + "AC"
    long1, long2 = (K, 1, "ACGTACGT", 5, -1), (K, 2, "GG", -1, 7)
    one = lambda ch, l=-1: (K, 1, ch, l, -1)                        # noqa: E731
    other = ("C" + K[1:], 1, "A", -1, -1)
    for run in ([long1, one("A")], [one("G"), one("C", 1), one("T"), one("C", 2)], [one("T"), long1, one("A"), long2, one("C")],
                [one("A"), one("A", 9)], [other, one("G"), long1], [one("C"), other, one("C")]):
        assert F.fold(run) == F.fold_closed_form(run), run
    assert F.fold([one("G"), one("C", 1), one("T"), one("C", 2)]) == [one("C", 2)]
    assert F.fold([one("T"), long1, one("A"), long2, one("C")]) == [long1, long2]


def test_the_crafted_rows_are_in_the_cases(cases):
    p, P, rows, st, ps, kmers, passes, text = cases["k41_P7_s2_M3"]
    mk = p["max_k"]
    total = lambda r: len(r.split(",")[0].lstrip("(")) + len(r.split(",")[2])     # noqa: E731
    assert {2 * mk - 1, 2 * mk, 2 * mk + 1} <= {total(r) for r in rows}
    assert len(st["binarized"]) < len(rows) and all(len(r[0]) + len(r[2]) >= 2 * mk for r in st["binarized"])
    assert {len(r[0]) + len(r[2]) for r in st["long"]} >= {60, 62, 63, 64, 65, 93, 94, 95, 96, 97}
    assert {r[1] for r in st["binarized"]} == {1, 2}
    sign = lambda v: (v > 0) - (v < 0)                              # noqa: E731
    assert {(sign(r[3]), sign(r[4])) for r in st["binarized"]} == {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)}
    assert any(abs(r[3]) == 30000 for r in st["binarized"]) and any("30001" in r for r in rows)
    assert any(r.startswith("(") for r in rows) and any("N" in r for r in rows)
    assert {r[3] for r in st["long"] if r[3] > 0} == {mk + 3} == {r[4] for r in st["long"] if r[4] > 0}
    from collections import Counter
    assert max(Counter(F.contig_of(r) for r in st["binarized"]).values()) == 2           # a contig and its duplicate
    assert len(set(kmers)) < len(kmers)                                                    # shared end 31-mers
    runs = Counter(r[0] for r in st["sort1"] if len(r[2]) == 1)
    assert max(runs.values()) == 4                                                         # all four bases behind one key
    keys_long = {r[0] for r in st["sort1"] if len(r[2]) > 1}
    assert any(r[0] in keys_long for r in st["sort1"] if len(r[2]) == 1)                   # a 31-mer on a trimmed contig's key
    assert any(len(F.contig_of(r)) >= 3000 for r in cases["k99_P63_s2_M0"][3]["binarized"])
    assert any(len(F.contig_of(r)) >= 3000 for r in cases["k31_P7_s3_M0"][3]["binarized"])
    # the loop really merges, in at least three different passes
    for n in ("k31_P1_s2_M150", "k32_P2_s3_M150", "k41_P7_s2_M3", "k99_P2_s2_M3"):
        c = cases[n]
        assert sum(1 for a, b in zip([c[3]["fold2"]] + c[6], c[6]) if len(b) < len(a)) >= 3, n


def test_the_vectors_regenerate_byte_for_byte(tmp_path):
    if not os.path.isdir(os.path.join(REF, "src", "main", "java")):
        pytest.skip("the reference's sources are not here")
    out = tmp_path / "fixing_vectors.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_fixing_vectors.py"), "--out", str(out)],
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
    assert [f for f, _ in _lib.CFixParams._fields_] == ["max_k", "scramble", "max_iteration"]
    L = _lib.lib()
    p = _lib.CFixParams()
    L.rfx_fix_default_params(p, 41)
    assert (p.max_k, p.scramble, p.max_iteration) == (41, 2, 150)
    src = open(os.path.join(ROOT, "reflexiv_amd", "csrc", "rfx_fixing.hip")).read()
    assert "rfx_fixing.hip" in open(os.path.join(ROOT, "reflexiv_amd", "csrc", "Makefile")).read()
    for name in SYMBOLS[1:]:
        body = src[src.index("int %s(" % name):]
        body = body[:body.index("RFX_API_CATCH")]
        assert "hipSetDevice(ctx->device)" in body and "hipDeviceSynchronize" not in body, name


def test_reflexiv_host_knows_fixing():
    from reflexiv_amd import _lib
    _lib.build()
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    assert os.path.exists(exe)
    r = subprocess.run([exe, "fixing"], capture_output=True, text=True)
    assert r.returncode != 0 and "-kmerc" in r.stderr + r.stdout and "-partition" in r.stderr + r.stdout
    r = subprocess.run([exe, "fixing", "-kmerc", "/nonexistent/part", "-outfile", "/nonexistent"], capture_output=True, text=True)
    assert r.returncode != 0
