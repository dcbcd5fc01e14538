"""tests/mercy_model.py against every stage the reference's own classes left in tests/golden/mercy_vectors.npz (made by
tests/golden/make_mercy_vectors.py: the seven operator classes of P/ReflexivDSDynamicMercyKmer.java translated from the reference's text
and driven in the driver's order, both union orders): the hit list per read, the kept ranges per read and the rows; and against a
planted genome, where the mercy rows are read from the GENOME.  No GPU."""
import os

import numpy as np
import pytest

from tests import mercy_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mercy_vectors.npz")


def strings(z, key):
    buf, off = bytes(z[key]), z[key + "_off"]
    return [buf[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


def load_case(z, name):
    """-> dict(rows, reads, k, fc, ec, hits per read, ranges per read as (left, right) = (a + 1, b), text, totals)"""
    k, fc, ec = (int(x) for x in z[name + "/params"])
    ho, ro = z[name + "/hits_off"], z[name + "/ranges_off"]
    hits, rng = z[name + "/hits"].tolist(), [tuple(x) for x in z[name + "/ranges"].tolist()]
    return dict(rows=[r.rstrip("\n") for r in strings(z, name + "/rows")], reads=strings(z, name + "/reads"), k=k, fc=fc, ec=ec,
                hits=[hits[ho[i]:ho[i + 1]] for i in range(len(ho) - 1)], ranges=[rng[ro[i]:ro[i + 1]] for i in range(len(ro) - 1)],
                text=bytes(z[name + "/text"]).decode(), totals=z[name + "/totals"].tolist())


@pytest.fixture(scope="module")
def vectors():
    return np.load(GOLDEN)


def case_names():
    return [str(n) for n in np.load(GOLDEN)["names"]] if os.path.exists(GOLDEN) else ["<tests/golden/mercy_vectors.npz is missing>"]


@pytest.mark.parametrize("name", case_names())
def test_model_equals_every_stage_of_the_reference(vectors, name):
    c = load_case(vectors, name)
    k, fc, ec = c["k"], c["fc"], c["ec"]
    solid = M.solid_set(c["rows"], k)
    hits = [M.hits(r, k, fc, ec, solid) for r in c["reads"]]
    # a read that gives nothing still has its hits in the reference's RamenReadExtraction (the filters sit behind it): compare the
    # hits of the reads that give something, and the ranges and the rows of all
    for i, r in enumerate(c["reads"]):
        if not M.gives_nothing(r, k, fc, ec):
            assert hits[i] == c["hits"][i], (name, i, r)
    ranges = [[(a + 1, b) for a, b in M.kept_ranges(h, k)] for h in hits]
    for i, r in enumerate(c["reads"]):
        if ranges[i] != c["ranges"][i]:
            # the reference keeps the ranges of a read whose blocks a later filter drops: such a read gives no rows either way
            assert M.gives_nothing(r, k, fc, ec) and ranges[i] == [], (name, i, r, ranges[i], c["ranges"][i])
    text = M.mercy_text(c["rows"], c["reads"], k, fc, ec)
    assert text == c["text"], name
    assert c["totals"][0] == len(c["reads"]) and c["totals"][3] == text.count("\n")


def test_vectors_cover_what_the_stage_can_meet(vectors):
    names = [str(n) for n in vectors["names"]]
    assert vectors["refused_k"].size == 0                          # the classes run at every k of 8..31
    assert {f"sweep_k{k}" for k in range(8, 32)} <= set(names)
    for k in (8, 15, 16, 21, 23, 30, 31):
        c = load_case(vectors, f"k{k}_c0_0")
        gaps = {r - l for rr in c["ranges"] for l, r in rr}         # right - left = b - a - 1
        want = {g for g in range(1, k + 4) if not k - 1 <= g <= k + 1}
        assert want <= gaps and not gaps & {k - 1, k, k + 1}, (k, sorted(want - gaps))
        assert c["totals"][3] > 0
        lens = {len(r) for r in c["reads"]}
        assert {k - 1, k, k + 1, k + 2, 16, 17, 18, 31, 32, 33, 63, 64, 65, 150, 151} <= lens
        assert any(r.startswith("A" * 31) and len(r) >= 32 for r in c["reads"]) and any("N" in r for r in c["reads"])
        assert any(r.startswith("(") for r in c["rows"]) and {len(r.split(",")[0].lstrip("(")) for r in c["rows"]} >= {k - 1, k, k + 3}
    for name in ("k21_front_clip_above_length", "k21_clips_leave_no_window"):
        assert load_case(vectors, name)["totals"][3] == 0
    for name in ("k15_c1_2", "k31_c1_2", "k21_clips_40_0", "k21_clips_0_40", "planted_k31"):
        assert load_case(vectors, name)["totals"][3] > 0


def test_planted_genome_rows_are_the_single_coverage_stretches(vectors):
    """a genome of 2,000 bases, reads of 100 at coverage >= 2 everywhere except two stretches that exactly one read crosses: with the
    k-mers seen twice as the solid set, the mercy rows are exactly the k-mers of the GENOME windows that touch a stretch"""
    c = load_case(vectors, "planted_k31")
    k = c["k"]
    genome = bytes(vectors["planted_k31/genome"]).decode()
    stretches = vectors["planted_k31/stretches"].tolist()
    assert len(genome) == 2000 and all(len(r) == 100 for r in c["reads"]) and len(stretches) == 2
    seen = {}
    for r in c["reads"]:
        for p in range(len(r) - k + 1):
            s = M.canon(r[p:p + k])
            seen[s] = seen.get(s, 0) + 1
    solid = {s for s, n in seen.items() if n >= 2}
    want = []
    for lo, hi in stretches:
        windows = [p for p in range(len(genome) - k + 1) if p + k > lo and p < hi]
        assert not k - 1 <= len(windows) <= k + 1                   # (the footprint of one substitution would be skipped)
        # coverage: every base of the stretch lies in exactly one read, every base outside in two or more
        want += [M.canon(genome[p:p + k]) for p in windows]
    cover = np.zeros(len(genome), int)
    for r in c["reads"]:
        at = genome.find(r) if genome.find(r) >= 0 else genome.find(M.rc(r))
        cover[at:at + len(r)] += 1
    inside = np.zeros(len(genome), bool)
    for lo, hi in stretches:
        inside[lo:hi] = True
    assert (cover[inside] == 1).all() and (cover[~inside] >= 2).all()
    got = M.mercy_kmers(c["reads"], k, 0, 0, solid)
    assert sorted(got) == sorted(want) and len(got) == sum(hi - lo + k - 1 for lo, hi in stretches)
    assert "".join(f"{s},1\n" for s in got) == c["text"]
    assert solid == M.solid_set(c["rows"], k)
