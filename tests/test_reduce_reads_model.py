"""The reduction from reads without a GPU: the composed string model (tests/reduce_reads_model.py) on the read sets
the device is held to in tests/test_gpu_reduce_reads_model.py.  What is asserted here are conditions on the INPUTS, which the model alone
must meet: the `forked` reads separate the E rule from every wrong rule listed, `doubled` overflows the driver's first count at every k
and `forked` never does, `edges` shows both counters' skip rules, `sensitive` brings mercy rows; and the vectors regenerate byte for
byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import reduce_reads_model as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "reduce_reads_vectors.npz")

# list -> (what the rule gives, the wrong rules run on purpose, the index of the Count_<k>_reduced in which each must differ)
SEPARATES = {
    (23, 67, 95): ([8, 6, 6], ([8, 8, 8], [8, 6, 8], [8, 8, 6]), 2),
    RR.DEFAULT_LIST: ([8, 8, 8, 8, 6, 6, 6], ([8] * 7, [8, 8, 8, 8, 6, 8, 8]), 6),
    (65, 81): ([8, 6], ([8, 8], [6, 6]), 1),                      # (the first-k quirk: 65 >= 61 but the second k is not below 81)
    (53, 67): ([8, 6], ([8, 8],), 1),
    (81, 95): ([6, 6], ([8, 8],), 1),
}


@pytest.fixture(scope="module")
def vectors():
    return RR.load_vectors(VEC)


def test_the_e_rule_as_the_orchestrator_writes_it():
    for klist, (want, _, _) in SEPARATES.items():
        assert RR.e_rule(klist, 2, 8) == want, klist
    assert RR.e_rule((31, 33), 2, 8) == [8, 8] and RR.e_rule((61, 80), 2, 8) == [6, 6] and RR.e_rule((61, 81), 2, 8) == [8, 6]
    assert RR.e_rule((60, 61), 2, 8) == [8, 6] and RR.e_rule((80, 95), 2, 8) == [8, 6] and RR.e_rule((81, 95), 3, 8) == [9, 9]
    assert RR.e_rule((31, 41, 67), 3, 8) == [8, 8, 9] and RR.e_rule((31, 41, 67), 2, 5) == [5, 5, 6]


def test_a_key_of_either_counter_reads_as_its_letters():
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    for k in (8, 23, 31, 33, 65, 95, 97, 124):
        s = RR.rnd(rng, k)
        if k <= 31:                                             # (a read of k bases gives no row at k <= 31: two bases more, the first window)
            key = O.extract_canon(*RR._flat([s + "AC"]), k)[0]
        else:
            key = O.extract_canon_w(*RR._flat([s]), k)[0]
        got = RR.key_letters(key, k)
        rc = s.translate(str.maketrans("ACGT", "TGCA"))[::-1]
        assert got in (s, rc) and (k > 31 or got == min(s, rc)), k


@pytest.mark.parametrize("klist", list(SEPARATES), ids=lambda l: "k" + "_".join(map(str, l)))
def test_the_forked_reads_separate_the_rule_from_the_wrong_rules(vectors, klist):
    reads, texts, _ = vectors
    rule, wrongs, where = SEPARATES[klist]
    info = {}
    good = RR.model(reads["forked"], klist, info=info, P=8)
    assert info["Es"] == rule
    assert good == texts["forked_k" + "_".join(map(str, klist)) + "_P8"]
    for w in wrongs:
        bad = RR.model(reads["forked"], klist, Es=w, P=8)
        assert bad[where] != good[where], f"the reads do not exercise the rule: E = {w} gives the same Count_{klist[where]}_reduced as E = {rule} on {klist}"


@pytest.mark.parametrize("tail", [40, 44])
def test_the_tail_of_the_three_extra_reads_must_start_at_36(tail):
    """with a later start the three extra instances miss k-mers that the pair (65, 81) needs: [8, 8] then gives what the rule gives"""
    assert RR.FORK_TAIL == 36
    reads = RR.forked_reads(tail)
    assert RR.model(reads, (65, 81), P=8) == RR.model(reads, (65, 81), Es=[8, 8], P=8)


def test_the_read_sets_are_the_recipes(vectors):
    reads = vectors[0]
    for name, fn in RR.READ_SETS.items():
        assert reads[name] == fn(), name
    f = reads["forked"]
    assert len(f) == 218 and 29000 < sum(len(r) for r in f) < 31000 and max(len(r) for r in f) == 30 + 150 - RR.FORK_TAIL + 30
    d = reads["doubled"]
    assert len(d) == 128 and d[0::2] == d[1::2] and len(set(d)) == 64 and min(len(r) for r in d) >= 96 and max(len(r) for r in d) == 150
    assert os.path.getsize(VEC) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "ksort_vectors.npz"))
    assert sorted(vectors[1]) == sorted(RR.cases())


def test_doubled_overflows_the_first_count_at_every_k_and_forked_never_does(vectors):
    """rr_sorted (reflexiv_amd/csrc/rfx_reduce.hip) counts into `inst / max(min_cov, 1) / 8 + 1024` rows first, inst = n_reads *
    max(max_read_len - k + 1, 0), and once more where the counter needs more: RR.first_capacity restates that formula"""
    reads, _, rows = vectors
    cases = RR.cases()
    for name, (rset, klist, kw) in cases.items():
        r = reads[rset]
        if not r:
            continue
        caps = [RR.first_capacity(len(r), max(len(x) for x in r), k, kw.get("min_cov", 2)) for k in klist]
        if rset == "doubled":
            assert all(n > c for n, c in zip(rows[name], caps)), (name, rows[name], caps)
        elif rset == "forked":
            assert all(n <= c for n, c in zip(rows[name], caps)), (name, rows[name], caps)
    # (the mercy reads overflow it by a few rows at k = 31 and 41 -- 1857 > 1794, 1827 > 1684 -- which is the one place the second count
    # ran before `doubled`: one-word and two-word keys, min_cov = 2; `doubled` adds the three- and four-word keys and min_cov = 1)
    s = reads["sensitive"]
    assert [n > RR.first_capacity(len(s), max(len(x) for x in s), k, 2) for n, k in zip(rows["sensitive"], (23, 31, 41))] == [False, True, True]
    assert rows["doubled"] == [6701, 6189, 5549, 3885, 2093]
    assert [RR.first_capacity(128, 150, k, 2) for k in RR.DOUBLED_LIST] == [2048, 1984, 1904, 1696, 1472]
    # min_cov = 1: every window is a row (each read is there twice, so the rows are the same), against a capacity twice as large
    assert rows["doubled_min_cov1"] == rows["doubled"][:3] and max(RR.DOUBLED_ALL_LIST) < 61
    assert rows["doubled_min_cov1"] == [sum(len(x) - k + 1 for x in reads["doubled"][::2]) for k in RR.DOUBLED_ALL_LIST]


def test_edges_shows_both_skip_rules(vectors):
    """k <= 31: a read gives rows iff it has k + 2 bases or more (len - k <= 1 is skipped); k > 31: iff it has k bases or more"""
    reads, texts, rows = vectors
    e = reads["edges"]
    lens = [len(r) for r in e]
    assert set(RR.edge_read_lengths()) <= set(lens) and {96, 128} <= set(lens)
    for k in RR.EDGES_LIST:
        for d in (-1, 0, 1, 2):
            pair = [r for r in e[40:] if len(r) == k + d]
            assert len(pair) >= 2 and len(set(pair)) == 1, (k, d)
            want = max(d + 1, 0) if k > 31 else (d + 1 if d >= 2 else 0)
            assert len(RR.counter_rows(pair[:2], k)) == want, (k, d)
    assert len(RR.counter_rows([r for r in e if len(r) == 31][:2], 31)) == 0          # a read of 31 bases gives no 31-mer
    assert len(RR.counter_rows([r for r in e if len(r) == 33][:2], 33)) == 1          # a read of 33 bases gives one 33-mer
    # and in the whole set: the rows of the ragged reads are in the counter's rows of the case, or are not
    for k in RR.EDGES_LIST:
        all_rows = set(RR.counter_rows(e, k))
        assert len(all_rows) == rows["edges"][RR.EDGES_LIST.index(k)]
        for d in (0, 1, 2):
            pair = [r for r in e[40:] if len(r) == k + d][:2]
            mine = set(RR.counter_rows(pair, k))
            assert mine <= all_rows and (len(mine) > 0) == (k > 31 or d == 2), (k, d)
    assert all(t.count("\n") > 0 for t in texts["edges"])


def test_sensitive_adds_mercy_rows_and_changes_the_texts(vectors):
    reads, texts, _ = vectors
    info = {}
    got = RR.model(reads["sensitive"], (23, 31, 41), info=info, P=8, sensitive=1)
    assert got == texts["sensitive"]
    assert info["mercy"][0] > 0 and info["mercy"][1] > 0 and info["mercy"][2] == 0       # (no mercy stage above 31)
    assert got != RR.model(reads["sensitive"], (23, 31, 41), P=8)


def test_no_reads_give_empty_texts(vectors):
    assert RR.model([], (23, 31, 41)) == ["", "", ""] == vectors[1]["none"]


def test_every_text_is_rows_of_its_k(vectors):
    _, texts, _ = vectors
    for name, (rset, klist, kw) in RR.cases().items():
        assert len(texts[name]) == len(klist)
        for k, t in zip(klist, texts[name]):
            assert all(len(row.split(",")[0]) == k and row.count("|") == 2 for row in t.splitlines()), (name, k)


def test_the_vectors_regenerate_byte_for_byte(tmp_path):
    out = tmp_path / "reduce_reads_vectors.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_reduce_reads_vectors.py"), "--out", str(out), "--jobs", "8"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert out.read_bytes() == open(VEC, "rb").read()
