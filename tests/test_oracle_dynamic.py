"""The dynamic-k record format and passes: the oracle (oracle/reflexiv_dynamic.c) against vectors made by
the REFERENCE'S OWN classes of P/ReflexivDSDynamicKmerFirstFour.java and P/ReflexivDSDynamicKmerIteration.java
(tests/golden/dynamic_vectors.npz, written by tests/golden/make_dynamic_vectors.py through tools/java2py.py): the rows after
EVERY operator of both drivers, keys of mixed lengths (k in 23..95), P in {1, 2, 3}, start iterations below and above 61."""
import os

import numpy as np
import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
VEC = os.path.join(HERE, "golden", "dynamic_vectors.npz")


def cases():
    z = np.load(VEC)
    return sorted({k.split("/")[0] for k in z.files})


def rows_of(z, name):
    text = bytes(z[name]).decode()
    return [tuple(ln.split(",")) for ln in text.split("\n") if ln]


@pytest.mark.parametrize("case", cases())
def test_dynamic_passes_equal_the_reference_classes(case):
    z = np.load(VEC)
    P, start, end = (int(x) for x in z[case + "/meta"])
    in_rows = rows_of(z, case + "/in")
    ff, tr1 = O.dyn_first_four(in_rows, P)
    for tag, rows in tr1:
        want = rows_of(z, f"{case}/{tag}")
        assert rows == want, (case, tag, next((i, a, b) for i, (a, b) in enumerate(zip(rows, want)) if a != b) if len(rows) == len(want)
                              else (len(rows), len(want)))
    fin, tr2 = O.dyn_iterations(ff, P, start, end)
    for tag, rows in tr2:
        want = rows_of(z, f"{case}/{tag}")
        assert rows == want, (case, tag, next((i, a, b) for i, (a, b) in enumerate(zip(rows, want)) if a != b) if len(rows) == len(want)
                              else (len(rows), len(want)))
    assert fin == rows_of(z, case + "/final")


# ---- the edge vectors: crafted families through the reference's own classes (tests/golden/make_dynamic_edge_vectors.py) ----
EDGE = os.path.join(HERE, "golden", "dynamic_edge_vectors.npz")


def edge_cases():
    z = np.load(EDGE)
    return sorted({k.split("/")[0] for k in z.files})


def first_difference(rows, want):
    if len(rows) != len(want):
        return len(rows), len(want)
    return next(((i, a, b) for i, (a, b) in enumerate(zip(rows, want)) if a != b), None)


def model_records(rows):
    """text rows -> the string model's records (tests/pymodel.py)"""
    out = []
    for k, a, e in rows:
        m, l, r = (int(x) for x in a.split("|"))
        out.append((k, m, e, l, r))
    return out


def model_rows(recs):
    return [(k, f"{m}|{l}|{r}", e) for k, m, e, l, r in recs]


@pytest.mark.parametrize("case", edge_cases())
def test_dynamic_passes_equal_the_reference_classes_on_crafted_families(case):
    """keys of 22..94 bases at the block edges (31, 32, 61, 62, 63, 92, 93), both markers, every distance branch with keys of
    different lengths, the rules from iteration 61 on, the +-30000 clamp, the emission marker starting at 1: the oracle's sort,
    cut and pass against the rows the reference's classes gave, each pass fed with the reference's previous output"""
    z = np.load(EDGE)
    P, stage, start, start_marker, passes = (int(x) for x in z[case + "/meta"])
    prev = rows_of(z, case + "/in")
    assert {len(r[0]) for r in prev} >= {22, 30, 31, 32, 40, 61, 62, 63, 80, 92, 93, 94}
    for i in range(passes):
        r = O.dyn_sort(O.dyn_binarize_rows(prev))
        g, ops = O.dyn_extend_pass(r, O.dyn_partition_starts(r, P), stage, start, start_marker)
        want = rows_of(z, f"{case}/pass{i}")
        assert g.rows() == want, (case, i, first_difference(g.rows(), want))
        assert ops[0] == 0 and ops[-1] == len(want) and np.all(np.diff(ops) >= 0)
        prev = want


@pytest.mark.parametrize("case", edge_cases())
def test_string_model_equals_the_reference_classes_on_crafted_families(case):
    """the string model of tests/pymodel.py (block order, cut, flip, merge, walk) against the same rows; its census of the first
    pass shows every decision the configuration can reach"""
    from tests import pymodel as M
    z = np.load(EDGE)
    P, stage, start, start_marker, passes = (int(x) for x in z[case + "/meta"])
    prev = rows_of(z, case + "/in")
    for i in range(passes):
        s = M.dyn_sort(model_records(prev))
        out, ops, labels = M.dyn_extend_pass(s, M.dyn_partition_starts(s, P), stage, start, start_marker)
        want = rows_of(z, f"{case}/pass{i}")
        assert model_rows(out) == want, (case, i, first_difference(model_rows(out), want))
        assert set(labels) <= set(M.dyn_labels(stage, start) + M.DYN_LABELS_EXTRA_DECIDES)
        if i == 0:
            census = M.dyn_census(labels)
            assert min(census.get(lb, 0) for lb in M.dyn_labels(stage, start)) >= 3, sorted(census.items())
        prev = want


@pytest.mark.parametrize("case", cases())
def test_string_model_equals_the_reference_classes(case):
    """the string model against the vectors cut from a genome (dynamic_vectors.npz): random reflection, the four first passes
    and every iteration, each fed with the reference's previous output"""
    from tests import pymodel as M
    z = np.load(VEC)
    P, start, end = (int(x) for x in z[case + "/meta"])
    recs = [(k[:-1], 1, k[-1], int(a.split("|")[1]), int(a.split("|")[2])) for k, a in rows_of(z, case + "/in")]
    assert model_rows(recs) == rows_of(z, case + "/binarized")
    n = len(recs)
    got = model_rows(M.dyn_random_reflection(recs, [p * n // P for p in range(P)] + [n]))
    assert got == rows_of(z, case + "/random_reflection"), first_difference(got, rows_of(z, case + "/random_reflection"))
    chain = [("random_reflection" if i == 0 else f"extend{i - 1}", f"extend{i}", 0) for i in range(4)]
    chain += [("it_binarized" if i == start + 1 else f"it_extend{i - 1}", f"it_extend{i}", 1) for i in range(start + 1, end + 2)]
    for src, dst, stage in chain:
        s = M.dyn_sort(model_records(rows_of(z, f"{case}/{src}")))
        out, _, _ = M.dyn_extend_pass(s, M.dyn_partition_starts(s, P), stage, start)
        want = rows_of(z, f"{case}/{dst}")
        assert model_rows(out) == want, (case, dst, first_difference(model_rows(out), want))


def test_crafted_families_reach_the_rows_where_extra_alone_decides():
    """a distance that reaches past the partner's extension but not past the longer key's extra bases: the reference-made rows hold
    both kinds (the row forward, the row reflected), so `- extra` in the two distance conditions is checked against the reference"""
    from tests import pymodel as M
    z = np.load(EDGE)
    census = {}
    for case in edge_cases():
        P, stage, start, start_marker, _ = (int(x) for x in z[case + "/meta"])
        s = M.dyn_sort(model_records(rows_of(z, case + "/in")))
        for lb, c in M.dyn_census(M.dyn_extend_pass(s, M.dyn_partition_starts(s, P), stage, start, start_marker)[2]).items():
            census[lb] = census.get(lb, 0) + c
    assert all(census.get(lb, 0) >= 3 for lb in M.DYN_LABELS_EXTRA_DECIDES), census
