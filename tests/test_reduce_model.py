"""The k-mer reduction stage without a GPU: the string model (tests/reduce_model.py) equals every stage of every case the
reference's own classes made (tests/golden/reduce_vectors.npz), every branch of both adjustments is taken by the cases, the vectors
regenerate byte for byte, the header declares the entry points that _lib binds, and reflexiv_host knows `reduce`."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import reduce_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "reduce_vectors.npz")
REF = os.environ.get("RFX_REFERENCE", "/root/reference")
SYMBOLS = ["rfx_reduce_default_params", "rfx_dev_reduce_union", "rfx_dev_reduce_left_prepare", "rfx_dev_reduce_adjust",
           "rfx_dev_reduce_right_prepare", "rfx_dev_reduce_full_kmers", "rfx_dev_reduce_neutralize", "rfx_dev_reduce_run", "rfx_reduce_text"]
PAIRS = ((8, 9), (23, 31), (30, 31), (31, 41), (33, 34), (53, 67), (64, 65), (95, 97), (97, 124))


def names():
    return [str(x) for x in np.load(VEC)["names"]]


def test_the_cases_are_the_ones_the_stage_is_pinned_on():
    z = np.load(VEC)
    metas = [R.load_case(z, n)[0] for n in names()]
    assert {(m["k1"], m["k2"]) for m in metas} == set(PAIRS)
    for k1, k2 in PAIRS:                                             # both names of the second output
        mk = {m["max_k"] for m in metas if (m["k1"], m["k2"]) == (k1, k2)}
        assert k2 in mk and any(x > k2 for x in mk)
    assert {m["P"] for m in metas} == {1, 2, 7, 63}
    assert {m["P"] for m in metas if (m["k1"], m["k2"]) == (23, 31)} == {1, 2, 7, 63}
    assert os.path.getsize(VEC) < (1 << 20)
    # where k or k - 1 is a multiple of 31 the classes of this stage agree with the string model: no pair is refused for it
    pr = z["probe_k"]
    assert {int(k) for row in pr for k in row[:2]} >= {31, 32, 62, 63, 93, 94}
    assert all(int(ok) == 1 and R.supported_pair(int(a), int(b)) for a, b, ok in pr), pr.tolist()
    assert not R.supported_pair(31, 31) and not R.supported_pair(41, 31) and not R.supported_pair(7, 31) and not R.supported_pair(31, 125)


def test_every_branch_of_both_adjustments_is_taken():
    z = np.load(VEC)
    assert len(z["branch_names"]) == 55 and all(int(h) > 0 for h in z["branch_hits"]), dict(zip(z["branch_names"], z["branch_hits"]))
    hits = {}
    for n in names():
        meta, rs, rl, st, ps, t1, t2 = R.load_case(z, n)
        if meta["max_k"] == meta["k2"]:
            R.run_stages(rs, rl, meta["k1"], meta["k2"], meta["P"], hits)
    assert [hits.get(str(b), 0) for b in z["branch_names"]] == [int(h) for h in z["branch_hits"]]


@pytest.mark.parametrize("case", names())
def test_the_model_equals_every_stage_of_the_reference(case):
    meta, rs, rl, st, ps, t1, t2 = R.load_case(np.load(VEC), case)
    got, gps = R.run_stages(rs, rl, meta["k1"], meta["k2"], meta["P"])
    for s in R.STAGES:
        assert got[s] == st[s], (case, s, next(i for i, (a, b) in enumerate(zip(got[s] + [None], st[s] + [None])) if a != b))
    assert gps == ps
    assert (R.to_text(got["neutral"], meta["k1"]), R.to_text(got["neutral"], meta["k2"])) == (t1, t2)
    assert all(len(v) == meta["P"] + 1 for v in ps.values())
    if meta["P"] == 63:
        assert any(a == b for a, b in zip(ps["left_sort"], ps["left_sort"][1:]))           # empty partitions
    # no operator emits more rows than it reads
    assert len(st["left_adj"]) <= len(st["left_sort"]) and len(st["right_adj"]) <= len(st["right_sort"]) and len(st["neutral"]) <= len(st["full"])
    assert R.handover(t2) == [(r[0][:-1], r[0][-1], 1, r[3], r[4]) for r in st["neutral"] if len(r[0]) == meta["k2"]]


def test_the_crafted_rows_are_in_the_cases():
    from collections import Counter
    meta, rs, rl, st, ps, t1, t2 = R.load_case(np.load(VEC), "k31_41_P63")
    assert max(Counter(r.split(",")[0] for r in rs).values()) == 40                        # the neutralizer's drop stretch
    dup = Counter(r.split(",")[0] for r in rs).most_common(1)[0][0]
    assert any(r.startswith(dup) for r in rl) and dup + "," not in t1
    assert any(r.startswith("(") and r.endswith(")") for r in rs) and any("30001" in r for r in rl)
    assert any(len(r.split(",")[0]) not in (31, 41) for r in rs + rl) and any("N" in r for r in rs)
    assert all(len(r[0]) in (31, 41) for r in st["union"])
    assert any(r[3] < 0 for r in st["union"]) and any(r[4] < 0 for r in st["union"])
    # an adjustment edits: an extension taken over, a marker set to -1
    before = Counter((r[0], r[1]) for r in st["left_sort"])
    assert any((r[0], r[1]) not in before for r in st["left_adj"])


def test_the_partition_cuts_change_the_result():
    """the window's state does not reset at a new key, so P is part of the stage's contract"""
    z = np.load(VEC)
    texts = {P: R.load_case(z, f"k23_31_P{P}")[5:] for P in (1, 2, 7, 63)}
    assert len({t for t in texts.values()}) > 1


def test_the_vectors_regenerate_byte_for_byte(tmp_path):
    if not os.path.isdir(os.path.join(REF, "src", "main", "java")):
        pytest.skip("the reference's sources are not here")
    out = tmp_path / "reduce_vectors.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_reduce_vectors.py"), "--out", str(out)],
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
    assert [f for f, _ in _lib.CReduceParams._fields_] == ["k1", "k2", "max_k"]
    L = _lib.lib()
    p = _lib.CReduceParams()
    L.rfx_reduce_default_params(p, 31, 41)
    assert (p.k1, p.k2, p.max_k) == (31, 41, 95)
    src = open(os.path.join(ROOT, "reflexiv_amd", "csrc", "rfx_reduce.hip")).read()
    assert "rfx_reduce.hip" in open(os.path.join(ROOT, "reflexiv_amd", "csrc", "Makefile")).read()
    assert '#include "rfx_reduce_fsm.h"' in src
    for name in SYMBOLS[1:]:
        body = src[src.index("int %s(" % name):]
        body = body[:body.index("RFX_API_CATCH")]
        assert "hipSetDevice(ctx->device)" in body and "hipDeviceSynchronize" not in body, name


def test_reflexiv_host_knows_reduce():
    from reflexiv_amd import _lib
    _lib.build()
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    assert os.path.exists(exe)
    r = subprocess.run([exe, "reduce"], capture_output=True, text=True)
    assert r.returncode != 0 and "-kmerc2" in r.stderr + r.stdout and "-kmer2" in r.stderr + r.stdout and "-partition" in r.stderr + r.stdout
    r = subprocess.run([exe, "reduce", "-kmerc", "a.csv", "-kmerc2", "b.csv", "-kmer", "41", "-kmer2", "31", "-outfile", "/nonexistent"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "41" in r.stderr + r.stdout
