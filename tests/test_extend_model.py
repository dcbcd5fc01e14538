"""The contig extension stages without a GPU: the string model (tests/extend_model.py -- its two own steps, then tests/fixing_model.py
and tests/fixing2_model.py unchanged) equals every stored stage of every case the reference's own classes made
(tests/golden/extend_vectors.npz); the device's view of the input (bases without the literals, and flags) gives the same end 31-mers
and long records as the text; what the reference throws on and what deviation 1 refuses; the cases cover what the stages are pinned
on; the vectors regenerate byte for byte; and the header, the bindings, the Makefile and reflexiv_host know the stages."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import extend_model as X
from tests import fixing_model as F
from tests import fixing2_model as F2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "extend_vectors.npz")
REF = os.environ.get("RFX_REFERENCE", "/root/reference")
SYMBOLS = ["rfx_dev_ext_from_text", "rfx_dev_ext_contig_ends", "rfx_dev_ext_run", "rfx_ext_text", "rfx_dev_ext2_to_text", "rfx_ext2_text"]


@pytest.fixture(scope="module")
def cases():
    z = np.load(VEC)
    return {n: X.load_case(z, n) for n in X.case_names()}


@pytest.mark.parametrize("case", X.case_names())
def test_the_model_equals_every_stored_stage(cases, case):
    p, P, rows, st, ps, kmers, passes, text, rounds2, text2 = cases[case]
    hits = {}
    mst, mps, mk, mpasses = X.run_stages(rows, p, P, hits)
    assert mk == kmers
    for s in X.STAGES:
        assert mst[s] == st[s], s
        if s in ps:
            assert mps[s] == ps[s], s
    assert mpasses == passes and X.to_text(mpasses[-1]) == text == X.run_text(rows, p, P)
    # the device's ascending order of the distinct 31-mers changes nothing from the first fold on
    sst, sps, _, spasses = X.run_stages(rows, p, P, order="sorted")
    assert sorted(sst["union"]) == sorted(st["union"])
    for s in ("fold1", "reflected", "sort2", "fold2"):
        assert sst[s] == st[s] and sps.get(s) == ps.get(s), s
    assert spasses == passes
    for q in range(P):
        for a, b in (("sort1", "fold1"), ("sort2", "fold2")):
            assert F.fold_closed_form(st[a][ps[a][q]:ps[a][q + 1]]) == st[b][ps[b][q]:ps[b][q + 1]]
    # 09ExtendAgain on the text of 08
    recs, mrounds, cs, mtext2 = X.run2_stages(text.splitlines(), p, P)
    assert mrounds == rounds2 and len(rounds2) == F2.loop_rounds(p)
    assert mtext2 == text2 and all(len(c[0]) >= 2 * p["max_k"] for c in cs)
    assert [ln.split(",")[0] for ln in text2.splitlines()] == [f">Contig-{len(c[0])}-{i}" for i, c in enumerate(cs)]


@pytest.mark.parametrize("case", X.case_names())
def test_the_devices_view_gives_the_same_ends_as_the_text(cases, case):
    p, P, rows, st, ps, kmers, *_ = cases[case]
    for in_flags in (True, False):
        dev = X.device_set(rows, p, in_flags)
        assert [X.set_text_chars(c) for c in dev] == [r[0] + r[2] for r in st["binarized"]]
        assert X.set_contig_ends(dev, p) == (st["long"], kmers)
        assert all(c["flags"] == 0 for c in dev) or in_flags
    assert all("l" not in c["bases"] and "-" not in c["bases"] for c in X.device_set(rows, p))


def test_the_cases_are_the_ones_the_stages_are_pinned_on(cases):
    assert os.path.getsize(VEC) <= 1.25 * os.path.getsize(os.path.join(ROOT, "tests", "golden", "fixing2_vectors.npz"))
    assert {c[0]["max_k"] for c in cases.values()} == {31, 32, 41, 99} and {c[1] for c in cases.values()} == {1, 2, 7, 63}
    assert {c[0]["scramble"] for c in cases.values()} == {2, 3} and {c[0]["max_iteration"] for c in cases.values()} == {0, 3, 150}
    flags, overlaps, ll, rl, cuts, lefts = set(), set(), set(), set(), set(), set()
    for p, P, rows, st, *_ in cases.values():
        dev = X.device_set(rows, p)
        flags |= {c["flags"] for c in dev}
        overlaps |= X.seam_overlaps(dev, p)
        ll |= {c["left_len"] for c in dev}
        rl |= {c["right_len"] for c in dev}
        cuts |= {len(r[0]) + len(r[2]) for r in st["long"]}
        lefts |= {X.parse_row(r)[0][1] for r in rows} | {X.parse_row(r)[0][2] for r in rows}
    assert flags == {0, 1, 2, 3} and overlaps == {(s, n) for s in "LR" for n in (1, 2, 3)}
    for ends in (ll, rl):
        assert {0, 1, 2, 3, 4, 30, 31, 32, 33, 300, 303} <= ends
    assert {32, 33, 61, 62, 63, 64, 65} <= cuts and max(cuts) >= 3000
    assert {30000, -30000, 30001, -30001, 0, 1, 2} <= lefts and min(lefts) < 0
    p, P, rows, st, ps, kmers, passes, text, rounds2, text2 = cases["k31_P1_s2_M150"]
    conts = [F.contig_of(r) for r in st["long"]]
    assert len(conts) != len(set(conts))                           # a contig and its duplicate
    assert len(kmers) != len(set(kmers))                           # two contigs sharing an end 31-mer
    assert {k[:30] for k in kmers} & {r[0] for r in st["long"]}    # an end 31-mer on a cut contig's key
    assert len(X.binarize(rows, p)) == len(rows) - 1               # one row a character below 2 max_k, one at it
    assert min(len(r[0]) + len(r[2]) for r in st["binarized"]) == 2 * p["max_k"]
    assert any(v < 0 for r in rows for v in (X.parse_row(r)[0][3], X.parse_row(r)[0][6]))
    assert any(set(X.parse_row(r)[1]) - set("ACGT-1lr") for r in rows)
    assert any(c["left_len"] + c["right_len"] == 606 for c in X.device_set(rows, p))       # one contig's 31-mers cross a block
    for n in ("k31_P1_s2_M150", "k32_P2_s3_M150", "k41_P7_s2_M3", "k99_P2_s2_M3"):
        c = cases[n]
        assert sum(1 for a, b in zip([c[3]["fold2"]] + c[6], c[6]) if len(b) < len(a)) >= 3, n
    z = np.load(VEC)
    hits = dict(zip([str(x) for x in z["branch_names"]], [int(x) for x in z["branch_hits"]]))
    assert all(h > 0 for b, h in hits.items() if b[:2] in ("L ", "R "))


def test_what_the_reference_throws_on_and_what_deviation_one_refuses():
    p = X.default_params(31)
    good = ">Contig_70_-1_2_0_5_4_0," + "ACGTA" + "C" * 70 + "GGGG"
    assert X.binarize([good], p) == [("ACGTA" + "C" * 26, 1, "C" * 44 + "GGGG", -1, 2, 5, 4)]
    longs, kmers = X.contig_ends(X.binarize([good], p), p)
    assert len(kmers) == 9 and longs == [("C" * 30, 1, "C" * 40, -1, 2)]
    for bad in ("Contig_70_-1_2_0_5_4_0," + "A" * 80, ">Contig_70_-1_2_0_5_4," + "A" * 80, ">Contig_70_-1_2_0_5_4_0_1," + "A" * 80,
                ">Contig_70_-1_x_0_5_4_0," + "A" * 80, ">Contig_70_-1__0_5_4_0," + "A" * 80, ">Contig_70_-1_2_0_5_4_0" + "A" * 80,
                ">Contig_70_-1_2_0_5_4_0,(" + "A" * 80, ">Contig_70_-1_2_0_5_99999999999_0," + "A" * 80):
        with pytest.raises(ValueError):
            X.parse_row(bad)
    # deviation 1: a kept contig whose cut part is below 32 characters; 32 passes
    for cut, ok in ((31, False), (32, True), (0, False)):
        row = f">Contig_{cut}_0_0_0_40_40_0," + "A" * (80 + cut)
        if ok:
            assert [len(r[0]) + len(r[2]) for r in X.contig_ends(X.binarize([row], p), p)[0]] == [32]
        else:
            with pytest.raises(ValueError):
                X.contig_ends(X.binarize([row], p), p)
    for ll, rl in ((-1, 0), (0, -1), (304, 0), (0, 304)):
        with pytest.raises(ValueError):
            X.contig_ends(X.binarize([f">Contig_700_0_0_0_{ll}_{rl}_0," + "A" * 700], p), p)
    # a row below 2 max_k is dropped before any of it is judged
    assert X.contig_ends(X.binarize([">Contig_1_0_0_0_30_30_0," + "A" * 61], p), p) == ([], [])
    with pytest.raises(ValueError):
        X.set_contig_ends([dict(bases="A" * 80, left=0, right=0, left_len=2, right_len=0, flags=1, src_idx=0, new_idx=0)], p)
    with pytest.raises(ValueError):
        X.to_text2([("A" * X.LINE_MAX, 0, 0)])


def test_the_vectors_regenerate_byte_for_byte(tmp_path):
    if not os.path.isdir(os.path.join(REF, "src", "main", "java")):
        pytest.skip("the reference's sources are not here")
    out = tmp_path / "extend_vectors.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_extend_vectors.py"), "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert out.read_bytes() == open(VEC, "rb").read()


def test_the_header_declares_the_entry_points_and_the_bindings_hold_them():
    from reflexiv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "reflexiv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and name in _lib._DYN_PACKED_ARGS, name
    _lib.lib()
    assert "rfx_ctgext.hip" in open(os.path.join(ROOT, "reflexiv_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "reflexiv_amd", "csrc", "rfx_ctgext.hip")).read()
    for name in SYMBOLS:
        body = src[src.index("int %s(" % name):]
        body = body[:body.index("RFX_API_CATCH")]
        assert ") try {" in body and "hipDeviceSynchronize" not in body, name
        assert "hipSetDevice(ctx->device)" in body or "fx2_text_call(" in body, name
        assert re.search(r":\d+-\d+", src[:src.index("int %s(" % name)].rsplit("\n\n", 1)[-1]), name        # cites its reference lines
    import reflexiv_amd
    for name in ("ext_from_text", "ext_contig_ends", "ext_run", "ext_text", "ext2_to_text", "ext2_text"):
        assert callable(getattr(reflexiv_amd.Reflexiv, name)), name
    # the reuse the stage is built on: one definition of the fixing stage's tail, called from both stages
    fixing = open(os.path.join(ROOT, "reflexiv_amd", "csrc", "rfx_fixing.hip")).read()
    new = open(os.path.join(ROOT, "reflexiv_amd", "csrc", "rfx_ctgext.hip")).read()
    assert fixing.count("int rfx::fx_from_ends(") == 1 and fixing.count("fx_from_ends(") == 2 and src.count("fx_from_ends(") == 2
    for word in ("atomicMin", "sort_pairs", "dyn_sort", "dyn_pass", "k_fx_", "fx_cat32"):
        assert word not in new, word


def test_reflexiv_host_knows_both_subcommands():
    from reflexiv_amd import _lib
    _lib.build()
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    assert os.path.exists(exe)
    for cmd in ("extend", "extend2"):
        r = subprocess.run([exe, cmd], capture_output=True, text=True)
        assert r.returncode != 0 and "-kmerc" in r.stderr + r.stdout and "-partition" in r.stderr + r.stdout, cmd
        r = subprocess.run([exe, cmd, "-kmerc", "/nonexistent/part", "-outfile", "/nonexistent"], capture_output=True, text=True)
        assert r.returncode != 0, cmd
