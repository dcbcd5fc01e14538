"""The end extension of contigs from alignment rows without a GPU: the string model (tests/endext_model.py) equals every stored stage
of every case the reference's own classes made (tests/golden/endext_vectors.npz), the cases cover what the stage is pinned on, the
three-word order key sorts as the ID strings do, the vectors regenerate byte for byte (java2py's additions leave every older file as
it was: their own tests regenerate them), and the header declares the entry points that _lib binds."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import endext_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "endext_vectors.npz")
REF = os.environ.get("RFX_REFERENCE", "/root/reference")
SYMBOLS = ["rfx_dev_endext_consensus", "rfx_dev_endext_contigs", "rfx_dev_endext_to_text", "rfx_endext_text"]


def names():
    return [str(x) for x in np.load(VEC)["names"]]


@pytest.fixture(scope="module")
def cases():
    z = np.load(VEC)
    return {n: E.load_case(z, n) for n in names()}


@pytest.mark.parametrize("case", names())
def test_the_model_equals_every_stored_stage(cases, case):
    mk, ctext, lines, cons, spliced, text = cases[case]
    rows = E.split_rows(lines)
    assert E.consensus_rows(rows) == cons
    assert E.extend(E.contigs_of_text(ctext), cons) == spliced
    assert E.tag(spliced, mk) == text == E.run_text(ctext, lines, mk)
    # what the device holds -- per-contig consensus, bases without the literals, the arrays -- gives the same text
    contigs = E.contigs_of_text(ctext)
    assert E.set_text(E.device_set(contigs, lines, mk)) == text
    by = {}
    for ident, s in cons:
        by.setdefault(ident, {})[s[0]] = s[2:]
    for (ident, _), (lc, rc, f) in zip(contigs, E.device_consensus(contigs, lines)):
        want = by.get(ident, {"L": "", "R": ""})
        assert ("l1-" * (f & 1) + lc, "r1-" * (f >> 1) + rc) == (want["L"], want["R"]), ident


def test_the_cases_are_the_ones_the_stage_is_pinned_on(cases):
    assert os.path.getsize(VEC) <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                                       if f.endswith(".npz") and f != "endext_vectors.npz")
    cons = [s for c in cases.values() for _, s in c[3]]
    assert any(s.startswith("L-l1-") for s in cons) and any(s.startswith("R-r1-") for s in cons)
    assert sum(1 for s in cons if len(s) == 2 + 300) >= 6 and max(len(s) for s in cons) == 2 + 300      # j reaches 299, 300 and 301: all cut at 300
    facts = {}
    for mk, ctext, lines, *_ in cases.values():
        E.consensus_rows(E.split_rows(lines), facts)
    assert facts["tie"] and facts["cut"]
    mk, ctext, lines, cons, spliced, text = cases["crafted_k31"]
    ids = [s.split(",")[0] for s in spliced]
    short = [c for c in E.contigs_of_text(ctext) if len(c[1]) <= 1]                              # originals of one base and of none: no rows of the
    assert sorted(len(c[1]) for c in short) == [0, 1] and len(spliced) == len(E.contigs_of_text(ctext)) - 2     # output, though one has a consensus
    assert any(i == short[0][0] and len(s) > 50 for i, s in cons) or any(i == short[1][0] and len(s) > 50 for i, s in cons)
    assert ids != sorted(ids, key=lambda s: [int(x) for x in s.split("_")[1:5]])                # bytes and numbers disagree
    assert any(len(r.split("\t")) == 3 for r in lines) and any(len(r.split("\t")) > 4 for r in lines)
    known = {c[0] for c in E.contigs_of_text(ctext)}
    rows = E.split_rows(lines)
    assert any(E.name_parts(r[0])[0] not in known for r in rows)                                # a name that matches no contig
    assert known - {E.name_parts(r[0])[0] for r in rows}                                        # a contig without rows
    assert any(r[3] != r[3].upper() for r in rows) and any("N" in r[3] for r in rows)
    assert any("I" in r[2] and "D" in r[2] for r in rows)
    assert len(spliced) > text.count("\n") or len(cases["crafted_k50"][4]) > cases["crafted_k50"][5].count("\n")
    # every pair of codes ties somewhere: the consensus of the tie contig is the higher code of each pair
    tie = [s for i, s in cons if i.startswith("Contig_90_-1_-1_")]
    assert tie == ["L-CGTGTT", "R-CGTGTT"]
    # a flagged side turns a field of 1 or less into 1 and leaves 2
    heads = [s.split(",")[0] for s in spliced if "-1l" in s]
    assert {h.split("_")[2] for h in heads} == {"1", "2"}


def test_what_the_reference_throws_on_the_model_refuses():
    good = ("Contig_100_0_0_0", "1", "10S50M", "A" * 60)
    assert E.contributions(*good)[0] == "A" * 10
    for bad in (("Contig_100_0_0_0", "x", "10S50M", "A" * 60), ("Contig_100_0_0_0", "1", "10S50", "A" * 60), ("Contig_100_0_0_0", "1", "S50M", "A" * 60),
                ("Contig_100_0_0_0", "1", "10s50M", "A" * 60), ("Contig_100_0_0_0", "1", "", "A" * 60), ("Contig_100_0_0_0", "1", "10S50M", "A" * 9),
                ("Contig_100_0_0_0", "51", "50M10S", "A" * 9), ("Contig_100_0_0_0", "1", "1000000000S5M", "A" * 60)):
        with pytest.raises(ValueError):
            E.contributions(*bad)
    assert E.contributions("Contig_100_0_0_0", "51", "50M10S", "A" * 10)[1] == "A" * 10        # the whole of seq is in reach


def random_id(rng):
    def num(signed):
        digits = int(rng.integers(1, 11))
        v = int(rng.integers(0, 10 ** digits))
        v = min(v, 2 ** 31 - 1)
        return -v if signed and v and rng.random() < 0.4 else v
    return f"Contig_{min(num(False), 2 ** 30 - 1)}_{num(True)}_{num(True)}_{num(False)}"


def test_the_three_word_key_orders_as_the_strings_do():
    rng = np.random.default_rng(7)
    ids = list({random_id(rng) for _ in range(10000)} | {"Contig_100_0_0_1", "Contig_99_0_0_1", "Contig_99_0_0_10", "Contig_99_0_0_2",
                                                          "Contig_99_-1_0_2", "Contig_99_-10_0_2", "Contig_99_-2147483648_-2147483648_2147483647",
                                                          "Contig_1073741823_-2147483648_-2147483648_2147483647", "Contig_9_0_0_0", "Contig_90_0_0_0"})
    assert len(ids) >= 10000
    assert sorted(ids, key=E.order_key) == sorted(ids)
    assert all(0 <= w < 2 ** 64 for i in ids[:100] for w in E.order_key(i))


def test_full_sam_lines_give_the_four_columns():
    sam = ["@SQ\tSN:Contig_70_-1_-1_0\tLN:70", "r1\t0\tContig_70_-1_-1_0\t4\t60\t20S62M30S\t*\t0\t0\tACGT\tIIII\tNM:i:0",
           "r2\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII", "short\tline"]
    assert E.sam_to_rows(sam) == ["Contig_70_-1_-1_0\t4\t20S62M30S\tACGT"]


def test_the_vectors_regenerate_byte_for_byte(tmp_path):
    if not os.path.isdir(os.path.join(REF, "src", "main", "java")):
        pytest.skip("the reference's sources are not here")
    out = tmp_path / "endext_vectors.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_endext_vectors.py"), "--out", str(out)],
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
    assert "rfx_endext.hip" in open(os.path.join(ROOT, "reflexiv_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "reflexiv_amd", "csrc", "rfx_endext.hip")).read()
    for name in SYMBOLS:
        body = src[src.index("int %s(" % name):]
        body = body[:body.index("RFX_API_CATCH")]
        assert ") try {" in body and "hipSetDevice(ctx->device)" in body and "hipDeviceSynchronize" not in body, name
        assert re.search(r":\d+-\d+", src[:src.index("int %s(" % name)].rsplit("\n\n", 1)[-1]), name        # cites its reference lines
    import reflexiv_amd
    for name in ("endext_consensus", "endext_contigs", "endext_to_text", "endext_text"):
        assert callable(getattr(reflexiv_amd.Reflexiv, name)), name
