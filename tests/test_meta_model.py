"""The independent model of the call from reads to contigs (tests/meta_model.py), on the CPU: the stored vectors
(tests/golden/meta_vectors.npz) are what the model gives today; the partition rule as Pipelines.java writes it; and the CONDITIONS
under which the read sets exercise the call -- conditions on the model alone, not measurements: where one fails the input is to be
changed, not the condition.  One input need not meet every condition, but every condition is met by some input."""
import os

import numpy as np
import pytest

from tests import endext_model as E
from tests import map_model as M
from tests import meta_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "meta_vectors.npz")


@pytest.fixture(scope="module")
def vec():
    return MM.load_vectors(VEC)


def test_the_stored_vectors_are_what_the_model_gives():
    want, got = MM.build_vectors(), np.load(VEC)
    assert sorted(want) == sorted(got.files)
    for k in want:
        assert np.array_equal(want[k], got[k]), k


def test_the_partition_rule():
    """Pipelines.java:877-883, 914-921, 954-974 in Java's int arithmetic"""
    assert MM.p_rule(8) == (8, 8, 8, 8) and MM.p_rule(9) == (9, 9, 9, 9)
    assert MM.p_rule(10) == (10, 8, 6, 4) and MM.p_rule(11) == (11, 8, 6, 4) and MM.p_rule(13) == (13, 10, 7, 5)
    assert MM.p_rule(63) == (63, 50, 37, 25) and MM.p_rule(99) == (99, 79, 59, 39)
    assert MM.p_rule(100) == (100, 80, 60, 20) and MM.p_rule(999) == (999, 799, 599, 199) and MM.p_rule(1000) == (1000, 800, 600, 100)
    assert len(MM.JOBS) == 8 and all(b < 20 or a > 20 for a, b in MM.JOBS) and MM.JOBS[-1] == (61, 70)


def test_the_read_sets_are_within_the_sizes_the_tests_are_held_to(vec):
    assert set(vec) == {"k23_31_41_O8", "k23_31_41_O10", "k23_67_95_O10"}
    for name, v in vec.items():
        assert len(v[0]) < 1000 and all(100 <= len(r) <= 150 for r in v[0]), name
        assert 20 <= sum(len(r) for r in v[0]) / 3000 <= 32, name
    assert vec["k23_31_41_O8"][0] == vec["k23_31_41_O10"][0] and vec["k23_31_41_O8"][2] == 8 and vec["k23_31_41_O10"][2] == 10


def met_by(vec, cond):
    return [name for name, v in vec.items() if cond(v)]


def test_the_second_fixing_stage_holds_two_contigs_or_more(vec):
    assert met_by(vec, lambda v: v[6]["05FixingAgain"] >= 2) == list(vec)


def test_the_mapper_gives_rows_at_both_ends_on_both_strands(vec):
    def cond(v):
        hs = M.hits(E.contigs_of_text(v[5]["05FixingAgain"]), v[0])
        return {(h[1] & 1, h[2]) for h in hs} == {(0, 0), (0, 1), (1, 0), (1, 1)} and len(hs) == v[6]["hits"]
    assert met_by(vec, cond) == list(vec)


def test_the_end_extension_lengthens_a_contig(vec):
    def cond(v):
        ids = [r.split(",")[0].split("_") for r in v[5]["07EndExtend"].splitlines()]
        return any(int(f[5]) + int(f[6]) > 0 for f in ids)
    assert met_by(vec, cond) == list(vec)


def test_the_de_duplication_removes_a_contig(vec):
    assert met_by(vec, lambda v: v[6]["Assembly"] < v[6]["09ExtendAgain"]), "no case in which the de-duplication removes a contig"


def test_the_assembly_is_not_empty_at_the_cases_min_contig(vec):
    assert met_by(vec, lambda v: v[5]["Assembly"].startswith(">Contig-") and v[4]["min_contig"] == 100) == list(vec)


def test_the_rule_at_10_gives_another_text_than_10_throughout(vec):
    """(10, 8, 6, 4) against P = 10 at every stage: the stage named here is the one test_gpu_meta.py runs on the device"""
    named = {name: v[7].get("rule_stage") for name, v in vec.items() if v[2] >= 10}
    assert named == {"k23_31_41_O10": "01Iteration5_9", "k23_67_95_O10": "01Iteration5_9"}, named


def test_skipping_the_rule_of_iteration_61_changes_a_file(vec):
    """the job 61-70 run with start 51 (so that no pass drops the shorter forward records) changes 01Iteration61_70 or a later file"""
    late = MM.STAGES[MM.STAGES.index("01Iteration61_70"):]
    assert met_by(vec, lambda v: v[7]["skip61_stage"] in late), {name: v[7]["skip61_stage"] for name, v in vec.items()}
