"""The string model of the end mapping (tests/map_model.py) against its consumer, with no GPU.  The stage has no
reference to compare with, so two checks tie the model to what reads its rows: (1) every row is one tests/endext_model.py takes, and
the bases that model piles up for it are exactly the overhang computed directly from the placement; (2) on a planted genome -- contigs
cut out of it, error-free reads over all of it -- tests/endext_model.run_text on the model's rows extends every inner contig end by
the genome's own flanking bases: a comparison with the genome, not with any model output."""
import numpy as np

from tests import endext_model as E
from tests import map_model as M


def crafted():
    """contigs of every target shape and reads that hang over their ends in every way the rules name"""
    rng = np.random.default_rng(11)
    lens = [62, 199, 200, 399, 400, 401, 1000, 90]
    contigs = [(f"Contig_{L}_{i - 3}_{3 - i}_{i}", M.rand_seq(rng, L)) for i, L in enumerate(lens)]
    reads = []
    for _, b in contigs:
        L = len(b)
        for over in (1, 2, 40, 69, 119):
            for n in (100, 150, 260):
                if n - over >= 31:
                    reads.append(M.rand_seq(rng, over) + b[:n - over])                 # over the left end
                    reads.append(b[max(0, L - (n - over)):] + M.rand_seq(rng, over))   # over the right end
                    reads.append(M.revcomp(reads[-2]))
                    reads.append(M.revcomp(reads[-2]))
    short = contigs[0][1]
    reads.append(M.rand_seq(rng, 20) + short + M.rand_seq(rng, 20))                    # past both ends of a whole-contig target: no row
    reads.append(M.rand_seq(rng, 1) + short)                                           # exactly n - 1 long: a left row
    reads.append("N" + contigs[3][1][:60])
    mm = list(M.rand_seq(rng, 30) + contigs[4][1][:80])
    mm[30 + 25] = "A" if mm[30 + 25] != "A" else "C"                                   # a mismatch behind the seed
    mm[30 + 79] = "A" if mm[30 + 79] != "A" else "C"                                   # and in the last base of the overlap
    reads.append("".join(mm))
    return contigs, reads


def direct_overhang(hit):
    """what a row adds to the pile-ups, from the placement alone: the overhang outwards from the contig on the left, in read order on
    the right.  One base over a LEFT end adds nothing: the consumer computes clip - start and skips a row where that is 0
    (P/ReflexivDSDynamicKmerMapping.java :683-713, endext_model.contributions `o > 0`), and start is 1 here; the row is still written"""
    ri, e, strand, off, v, p, over, name, r, tlen = hit
    return ("", r[len(r) - over:]) if e & 1 else (r[:over][::-1] if over >= 2 else "", "")


def test_every_model_row_is_one_the_consumer_takes_and_adds_exactly_the_overhang():
    contigs, reads = crafted()
    hs = M.hits(contigs, reads)
    assert len(hs) > 150
    seen = set()
    for h in hs:
        name, start, cigar, seq = M.row_of(h).split("\t")
        assert E.CIGAR.fullmatch(cigar), cigar
        assert E.contributions(name, start, cigar, seq) == direct_overhang(h), M.row_of(h)
        assert h[6] >= 1 and h[4] >= 31 and len(seq) == len(M.norm(reads[h[0]]))
        seen.add((h[1] & 1, h[2], h[5] > 0, name[-2:] in ("-L", "-R")))
    # both sides, both strands, with and without a clip at the far end, whole-contig and 200-base targets
    assert {(s, t, False, w) for s in (0, 1) for t in (0, 1) for w in (False, True)} <= seen
    assert {(s, t, True, True) for s in (0, 1) for t in (0, 1)} <= seen and not any(p and not two for _, _, p, two in seen)
    # the order of the rows: read, strand, end, offset
    keys = [h[:4] for h in hs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    by_read = {}
    for h in hs:
        by_read.setdefault(h[0], []).append(h)
    n = len(reads)
    assert n - 4 not in by_read                                     # the both-ends rule
    assert [(h[1], h[3], h[4], h[5]) for h in by_read[n - 3]] == [(0, 1, 62, 0)]       # a target exactly n - 1 long
    assert by_read[n - 2][0][8][0] == "T"                           # an N reads as T, here and in the seq
    assert [(h[1], h[4]) for h in by_read[n - 1]] == [(8, 80)]      # two mismatches are taken
    assert M.hits(contigs, reads[-1:], max_mismatch=1) == []
    assert [h[:5] for h in M.hits(contigs, reads[-1:], seed=11, min_overlap=11)] == [(0, 8, 0, 30, 80)]


def test_the_rules_at_their_edges():
    rng = np.random.default_rng(12)
    T = M.rand_seq(rng, 100)
    contigs = [("Contig_100_0_0_0", T)]
    left = lambda n, over: M.rand_seq(rng, over) + T[:n - over]    # noqa: E731
    # v at min_overlap and one below it; overhang 1 and the largest that leaves min_overlap
    assert [h[3:7] for h in M.hits(contigs, [left(60, 29)])] == [(29, 31, 0, 29)]
    assert M.hits(contigs, [left(60, 30)]) == []
    assert [h[3:7] for h in M.hits(contigs, [left(32, 1)])] == [(1, 31, 0, 1)]
    # the shortest read that can hit has seed + 1 bases (an overhang of one base), given a min_overlap it can reach
    assert [h[3:5] for h in M.hits(contigs, [left(22, 1)], min_overlap=21)] == [(1, 21)]
    assert M.hits(contigs, [T[:21]], min_overlap=21) == [] and M.hits(contigs, ["A"]) == []
    # no overhang, no row: the seed at offset 0 of a left end, or at the read's end of a right end
    assert M.hits(contigs, [T[:60], T[40:]]) == []
    # a mismatch inside the seed gives no row
    r = list(left(80, 10))
    r[10 + 5] = "A" if r[10 + 5] != "A" else "C"
    assert M.hits(contigs, ["".join(r)]) == []
    # a palindromic seed: each strand on its own
    pal = "ACGTAGGCTA" + M.revcomp("ACGTAGGCTA")
    assert M.revcomp(pal) == pal
    c2 = [("Contig_70_0_0_0", pal + M.rand_seq(rng, 50))]
    got = M.hits(c2, ["GG" + c2[0][1][:60]], seed=20)
    assert (0, 0, 0, 2, 60) in [h[:5] for h in got]
    # a tandem repeat gives two offsets in one read
    unit = M.rand_seq(rng, 25)
    c3 = [("Contig_90_0_0_0", unit + unit + M.rand_seq(rng, 40))]
    got = M.hits(c3, ["C" + unit + unit + unit], max_mismatch=31)
    assert [h[2:5] for h in got if h[1] == 0] == [(0, 1, 75), (0, 26, 50)]


def test_planted_genome_every_inner_end_grows_by_the_genomes_own_flank():
    genome, spans, contigs, reads = M.planted_case()
    assert len(spans) >= 5 and all(40 <= b[0] - a[1] <= 120 for a, b in zip(spans, spans[1:]))
    assert {len(r) for r in reads} == {100, 150}
    max_k = 31
    text = E.run_text(M.contig_text(contigs), M.rows(contigs, reads), max_k)
    rows = {}
    for line in text.splitlines():
        ident, seq = line[1:].split(",")
        f = ident.split("_")
        rows[int(f[4])] = (int(f[5]), int(f[6]), seq)
    assert sorted(rows) == list(range(len(contigs)))
    for i, (s, e) in enumerate(spans):
        ll, rl, seq = rows[i]
        assert seq[ll:len(seq) - rl] == genome[s:e]
        if i > 0:                                                   # an inner left end
            assert ll > 0 and seq[:ll] == genome[s - ll:s], (i, "left")
            assert ll >= spans[i][0] - spans[i - 1][1] or ll >= 100, (i, ll)
        if i + 1 < len(spans):                                      # an inner right end
            assert rl > 0 and seq[len(seq) - rl:] == genome[e:e + rl], (i, "right")
            assert rl >= spans[i + 1][0] - spans[i][1] or rl >= 100, (i, rl)
