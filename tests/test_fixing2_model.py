"""The second contig fixing stage without a GPU: the string model (tests/fixing2_model.py) equals every round and both texts of
every case the reference's own classes made (tests/golden/fixing2_vectors.npz), the cases cover what the stage is pinned on,
the vectors regenerate byte for byte, and the header declares the entry points that _lib binds."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import fixing2_model as F
from tests import fixing_model as F1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "fixing2_vectors.npz")
REF = os.environ.get("RFX_REFERENCE", "/root/reference")
SYMBOLS = ["rfx_dev_fix2_binarize", "rfx_dev_fix2_run", "rfx_dev_fix2_contigs", "rfx_dev_fix2_to_text", "rfx_dev_fix2_ends_text", "rfx_fix2_text"]


def names():
    return [str(x) for x in np.load(VEC)["names"]]


@pytest.fixture(scope="module")
def cases():
    z = np.load(VEC)
    return {n: F.load_case(z, n) for n in names()}


def sizes(c):
    return [len(c[3])] + [len(x[2]) for x in c[4]]


def test_the_cases_are_the_ones_the_stage_is_pinned_on(cases):
    ps = [(c[0], c[1]) for c in cases.values()]
    assert {p["max_k"] for p, _ in ps} == {31, 32, 41, 99}
    assert {P for _, P in ps} == {1, 2, 7, 63}
    assert {p["scramble"] for p, _ in ps} == {2, 3}
    assert {p["max_iteration"] for p, _ in ps} == {-1, 0, 3, 27, 28, 150}
    assert {len(c[4]) for c in cases.values()} == {0, 1, 4, 28, 29}               # the cap of 29 rounds shows at 28 and at 150
    for p, P, rows, recs, passes, text, ends in cases.values():
        assert len(passes) == max(0, min(p["max_iteration"] + 1, 29)) == F.loop_rounds(p)
    assert os.path.getsize(VEC) < (1 << 20)
    # the nine outputs of the first stage are inputs, under their own parameters
    z1 = np.load(os.path.join(ROOT, "tests", "golden", "fixing_vectors.npz"))
    for n in z1["names"]:
        c = cases["fix_" + str(n)]
        assert "\n".join(c[2]) + "\n" == z1[str(n) + "/text"].tobytes().decode()
        assert [c[0]["max_k"], c[0]["scramble"], c[0]["max_iteration"], c[1]] == [int(x) for x in z1[str(n) + "/meta"][:4]]
    # empty partitions behind a loop pass
    assert any(P == 63 and any(a == b for a, b in zip(x[1], x[1][1:])) for p, P, rows, recs, passes, *_ in cases.values() for x in passes)


def test_the_conditions_the_generator_insists_on(cases):
    merging = {n: sum(1 for a, b in zip(sizes(c), sizes(c)[1:]) if b < a) for n, c in cases.items()}
    assert [merging[n] for n in names()] == [int(x) for x in np.load(VEC)["merging_rounds"]]
    assert sum(1 for m in merging.values() if m >= 3) >= 3
    for n in ("fix_k41_P7_s2_M3", "fix_k99_P2_s2_M3", "fix_k32_P1_s2_M3"):        # the first stage left them records to merge
        assert merging[n] == 4 == len(cases[n][4]), n
    lengths, dropped_before_kept = [], False
    for p, P, rows, recs, passes, text, ends in cases.values():
        last = passes[-1][2] if passes else recs
        kept = [len(F1.contig_of(r)) >= 2 * p["max_k"] for r in last]
        dropped_before_kept |= any(not a and any(kept[i + 1:]) for i, a in enumerate(kept))
        lengths += [(len(F1.contig_of(r)), p["max_k"]) for r in last]
    assert dropped_before_kept                                                      # so idx is the rank among the KEPT contigs
    assert any(L < 2 * mk for L, mk in lengths) and any(2 * mk <= L < 400 for L, mk in lengths) and any(L >= 400 for L, mk in lengths)
    assert any(L >= 3000 for L, mk in lengths)
    assert sum(1 for L, mk in lengths if L >= 400) >= 6


def test_the_crafted_rows_are_in_the_new_cases(cases):
    for n, c in cases.items():
        if not n.startswith("new_"):
            continue
        p, P, rows, recs = c[:4]
        mk = p["max_k"]
        L = {len(F1.contig_of(r)) for r in recs}
        assert {2 * mk - 1, 2 * mk, 2 * mk + 1, 399, 400, 401} <= L, n
        assert {len(r[2]) for r in recs} >= {1, 2, 31, 32, 33, 34, 63, 64, 65}, n
        assert {r[1] for r in recs} == {1, 2}
        for side in (3, 4):
            v = {r[side] for r in recs}
            assert {-30000, 30000, 0} <= v and any(-30000 < x < 0 for x in v) and any(0 < x < 30000 for x in v), (n, side)
        assert any(r.startswith("(") for r in rows), n
        assert all(len(r[0]) == 30 for r in recs)


@pytest.mark.parametrize("case", names())
def test_the_model_equals_every_round_and_both_texts_of_the_reference(cases, case):
    p, P, rows, recs, passes, text, ends = cases[case]
    got = F.run_passes(F.binarize(rows), p, P)
    assert len(got) == len(passes)
    for i, (a, b) in enumerate(zip(got, passes)):                 # the loop is the dynamic-k pass (pymodel.dyn_extend_pass), unchanged
        assert a[0] == b[0], (case, "sort", i)
        assert a[1] == b[1] and len(a[1]) == P + 1, (case, "partition starts", i)
        assert a[2] == b[2], (case, "pass", i)
    grecs, gpasses, cs, gtext, gends = F.run_stages(rows, p, P)
    assert grecs == recs and (gtext, gends) == (text, ends) == F.run_text(rows, p, P)
    # the texts' grammar, and the capacity bound of the contigs
    last = passes[-1][2] if passes else recs
    assert len(cs) <= len(last) and sum((len(c[0]) + 31) // 32 for c in cs) <= sum((len(r[2]) + 31) // 32 for r in last) + len(last)
    for i, (row, c) in enumerate(zip(text.splitlines(), cs)):
        assert row == f"Contig_{len(c[0])}_{c[1]}_{c[2]}_{i},{c[0]}" and len(c[0]) >= 2 * p["max_k"]
    assert text.count("\n") == len(cs)
    assert ends.count(">") == sum(2 if len(c[0]) >= 400 else 1 for c in cs) and ends.count("\n") == 2 * ends.count(">")
    assert all(len(b) <= len(a) for a, b in zip([recs] + [x[2] for x in passes], [x[2] for x in passes]))


def test_the_text_model_on_small_sets():
    p = F.default_params(31)
    a, b, c = "ACGT" * 100, "C" * 399, "G" * 61
    recs = [(c[:30], 1, c[30:], 1, 1), (a[:30], 1, a[30:], -1, 30000), (b[369:], 2, b[:369], -30000, 0), (c[:30], 1, c[30:] + "T", 5, -5)]
    cs = F.contigs(recs, p)
    assert cs == [(a, -1, 30000), (b, -30000, 0), ("G" * 61 + "T", 5, -5)]
    assert F.to_text(cs) == f"Contig_400_-1_30000_0,{a}\nContig_399_-30000_0_1,{b}\nContig_62_5_-5_2,{'G' * 61}T\n"
    assert F.ends_text(cs) == (f">Contig_400_-1_30000_0-L\n{a[:200]}\n>Contig_400_-1_30000_0-R\n{a[200:]}\n"
                               f">Contig_399_-30000_0_1\n{b}\n>Contig_62_5_-5_2\n{'G' * 61}T\n")
    assert F.loop_rounds(dict(max_iteration=-1)) == 0 and [F.loop_rounds(dict(max_iteration=m)) for m in (0, 3, 27, 28, 29, 150)] == [1, 4, 28, 29, 29, 29]
    with pytest.raises(ValueError):
        F.binarize(["ACGT,1|2|3,ACGT"])
    with pytest.raises(ValueError):
        F.binarize(["A" * 30 + ",1|2|3,"])


def test_the_vectors_regenerate_byte_for_byte(tmp_path):
    if not os.path.isdir(os.path.join(REF, "src", "main", "java")):
        pytest.skip("the reference's sources are not here")
    out = tmp_path / "fixing2_vectors.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_fixing2_vectors.py"), "--out", str(out)],
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
    assert "rfx_fixing2.hip" in open(os.path.join(ROOT, "reflexiv_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "reflexiv_amd", "csrc", "rfx_fixing2.hip")).read()
    for name in SYMBOLS:
        body = src[src.index("int %s(" % name):]
        body = body[:body.index("RFX_API_CATCH")]
        assert ("hipSetDevice(ctx->device)" in body or "fx2_text_call(" in body) and "hipDeviceSynchronize" not in body, name
    import reflexiv_amd
    for name in ("fix2_binarize", "fix2_run", "fix2_contigs", "fix2_to_text", "fix2_ends_text", "fix2_text"):
        assert callable(getattr(reflexiv_amd.Reflexiv, name)), name


def test_reflexiv_host_knows_fixing2():
    from reflexiv_amd import _lib
    _lib.build()
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    assert os.path.exists(exe)
    r = subprocess.run([exe, "fixing2"], capture_output=True, text=True)
    assert r.returncode != 0 and "fixing2 needs" in r.stderr and "-kmerc" in r.stderr and "-partition" in r.stderr
    r = subprocess.run([exe, "fixing2", "-kmerc", "/nonexistent/part", "-outfile", "/nonexistent"], capture_output=True, text=True)
    assert r.returncode != 0
