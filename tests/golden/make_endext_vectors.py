#!/usr/bin/env python3
"""Golden vectors for the end extension of contigs from alignment rows (Assembly_intermediate/07EndExtend) made by the REFERENCE'S
OWN classes.

The five classes of P/ReflexivDSDynamicKmerMapping.java that sit behind its aligner are translated mechanically (tools/java2py.py,
from the reference's source text at generation time) and driven in the driver's order (:305-347): SAMString2ROW -> sort("contig") ->
DSProcessSAMandExtendContigs -> union with OldContig2Row of 05FixingAgain -> sort("ID") -> DSExtendContigs -> zipWithIndex ->
TagStringContigRDDID.  What sits between two classes is Spark's: both sorts stable and in byte order of the string, the union
with the consensus rows first, and -- the stated deviation -- ALL alignment rows in ONE logical partition, one operator instance.
No reference code is stored.

Every stage is ALSO computed by the string model (tests/endext_model.py) and must agree.

Inputs: the 05FixingAgain texts of three cases of fixing2_vectors.npz with synthesized rows (reads that overhang the contig ends, as
an aligner would report them: soft clips, a start, noise, lower case, N), and crafted contigs with crafted rows for every edge of
the rules.  No aligner is needed.  The generator FAILS unless both flags occur, a tie is broken, the 300 cap cuts a row and at
least one pair of IDs is ordered differently by bytes and by numbers.

Output: tests/golden/endext_vectors.npz -- per case max_k, the contig text (a case named fix_<name> reads the text of case <name> of
fixing2_vectors.npz), the row text, the consensus rows ("ID\\tL-..." lines), the spliced strings and the text of 07EndExtend."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import java2py as jp  # noqa: E402
import endext_model as em  # noqa: E402
from make_reference_vectors import make_param, drain  # noqa: E402
from make_dedup_vectors import rand_seq  # noqa: E402
from make_fixing2_vectors import Tuple2  # noqa: E402

REF = os.environ.get("RFX_REFERENCE", "/root/reference") + "/src/main/java/uni/bielefeld/cmg/reflexiv/pipeline/"
CLASSES = ["SAMString2ROW", "DSProcessSAMandExtendContigs", "OldContig2Row", "DSExtendContigs", "TagStringContigRDDID"]
FIX2_CASES = (("new_k31_P2_s2_M-1", 31, 3), ("new_k99_P63_s2_M3", 99, 2), ("fix_k41_P7_s2_M3", 41, 4))      # (case, max_k, rows per end)
_cls = {}


def op(name, param):
    if not _cls:
        _cls.update(jp.translate_classes(REF + "ReflexivDSDynamicKmerMapping.java", CLASSES))
    return _cls[name](jp.Outer(param, _cls))


def ref_pipeline(contig_text, row_lines, max_k):
    """-> (the consensus rows, the spliced strings, the text of 07EndExtend)"""
    param = make_param(31)
    param.maxKmerSize = jp._I(max_k)
    rows = drain(op("SAMString2ROW", param).call(jp.JIter([r.rstrip("\n") for r in row_lines])))
    rows.sort(key=lambda r: r.vals[0].encode())                                        # sort("contig"): stable, ONE partition
    cons = drain(op("DSProcessSAMandExtendContigs", param).call(jp.JIter(rows)))
    old = drain(op("OldContig2Row", param).call(jp.JIter([jp.Row(r.split(",")) for r in contig_text.splitlines()])))
    union = sorted(cons + old, key=lambda r: r.vals[0].encode())                       # union, sort("ID"): stable
    strings = drain(op("DSExtendContigs", param).call(jp.JIter(union)))
    tagged = []
    for idx, s in enumerate(strings):                                                  # zipWithIndex
        tagged += drain(op("TagStringContigRDDID", param).call(Tuple2(s, jp._L(idx))))
    return [(r.vals[0], r.vals[1]) for r in cons], list(strings), "".join(f"{r.vals[0]},{r.vals[1]}\n" for r in tagged)


def noisy(rng, s):
    """a read's bases: one in 25 replaced by another letter, a lower-case letter or N"""
    out = list(s)
    for i in range(len(out)):
        u = rng.random()
        if u < 0.04:
            out[i] = "ACGTacgtNN"[int(rng.integers(0, 10))]
    return "".join(out)


def end_rows(rng, ident, bases, per_end):
    """rows of reads that overhang both ends of a contig, named as 06ContigEnds names them"""
    L = len(bases)
    two = L >= 2 * em.END
    ext_l, ext_r = rand_seq(rng, 340), rand_seq(rng, 340)          # what lies beyond the contig: ext_l[0] is the base next to it
    rows = []
    for _ in range(per_end):
        ref = bases[:em.END] if two else bases
        s, start, m = int(rng.integers(1, 150)), int(rng.integers(1, 13)), int(rng.integers(20, min(100, len(ref) - 12)))
        o = s - start
        clip = "".join(ext_l[o - i] if i <= o else ref[start - s + i - 1] for i in range(s))
        rows.append((ident + ("-L" if two else ""), start, f"{s}S{m}M", noisy(rng, clip + ref[start - 1:start - 1 + m])))
        ref = bases[L - em.END:] if two else bases
        s, tail, m = int(rng.integers(1, 150)), int(rng.integers(0, 13)), int(rng.integers(20, min(100, len(ref) - 12)))
        start = len(ref) - m - tail + 1
        clip = (ref[len(ref) - tail:] + ext_r)[:s]
        rows.append((ident + ("-R" if two else ""), start, f"{m}M{s}S", noisy(rng, ref[start - 1:start - 1 + m] + clip)))
    return rows


def crafted(rng, mk):
    """-> (contig text, row lines): one contig or a few per rule"""
    cs, rows = [], []

    def contig(L, left=-1, right=-1):
        bases = rand_seq(rng, L)
        cs.append((L, left, right, bases))
        return f"Contig_{L}_{left}_{right}_{len(cs) - 1}", bases

    def row(name, start, cigar, seq):
        rows.append((name, start, cigar, seq))

    # start 9 / 10 on the left, tail 9 / 10 on the right, on ends and on plain names
    for L in (450, 120):
        sfx = ("-L", "-R") if L >= 400 else ("", "")
        ref = 200 if L >= 400 else L
        for start in (9, 10):
            c, _ = contig(L)
            row(c + sfx[0], start, "40S50M", rand_seq(rng, 90))
        for tail in (9, 10):
            c, _ = contig(L)
            row(c + sfx[1], ref - 50 - tail + 1, "50M40S", rand_seq(rng, 90))
    # overhang minus start of 0 and 1 (left), overhang minus tail of 0 and 1 (right)
    c, _ = contig(130)
    row(c, 5, "5S50M", rand_seq(rng, 55))
    row(c, 75, "50M6S", rand_seq(rng, 56))                         # tail 6: o = 0
    c, _ = contig(130)
    row(c, 5, "6S50M", rand_seq(rng, 56))
    row(c, 75, "50M7S", rand_seq(rng, 57))                         # o = 1
    # overhangs that reach j = 299, 300 and 301 on both sides: the 300 cap
    for reach in (299, 300, 301):
        c, _ = contig(500)
        row(c + "-L", 1, f"{reach + 1}S40M", rand_seq(rng, reach + 41))
        row(c + "-R", 161, f"40M{reach + 1}S", rand_seq(rng, reach + 41))
    # I, D and a leading S before the first M; =, X, N and H count like M
    c, _ = contig(300)
    row(c, 3, "12S30M5I20M7D10M", rand_seq(rng, 77))
    row(c, 200, "5S50M2I10D40M20S", rand_seq(rng, 117))            # align 98: tail 300 - (98 + 199) = 3
    row(c, 195, "4H3S30M60=2X8N25S", rand_seq(rng, 120))           # the walk starts at the first M; =, X and N add: align 100, tail 6
    row(c, 1, "30S", rand_seq(rng, 30))                            # one operation: first and last
    # a plain row that feeds both sides
    c, b = contig(70)
    row(c, 4, "20S62M30S", rand_seq(rng, 20) + b[3:65] + rand_seq(rng, 30))
    row(c, 2, "9S66M11S", rand_seq(rng, 86).lower())
    row(c, 2, "9S66M11S", "N" * 86)
    row(c, 2, "9S66M11S", "acgtnACGTN*-" * 7 + "ac")
    # exact ties between every pair of codes, one position each
    c, _ = contig(90)
    row(c, 1, "6S40M", "GCCAAA" + rand_seq(rng, 40))
    row(c, 1, "6S40M", "TTGTGC" + rand_seq(rng, 40))
    row(c, 51, "40M6S", rand_seq(rng, 40) + "AAACCG")
    row(c, 51, "40M6S", rand_seq(rng, 40) + "CGTGTT")
    # repeat counts 1 and 2 per side, on every kind of name, with left / right of < 0, 0, 1 and 2
    for v in (-7, 0, 1, 2):
        c, _ = contig(95 + v, left=v, right=v)
        row(c, 0, "*", "L")
        row(c, 0, "*", "R")                                        # one of each: no flag
        c, _ = contig(96 + v, left=v, right=v)
        row(c, 0, "*", "L-R")
        row(c, 1, "", "L")                                         # left 2, right 1
        row(c, 3, "10S60M", rand_seq(rng, 70))
        c, _ = contig(460 + v, left=v, right=v)
        row(c + "-R", 0, "*", "R")
        row(c + "-R", 0, "*", "R")                                 # right 2
        row(c + "-L", 0, "*", "L")
        row(c + "-L", 2, "30S60M", rand_seq(rng, 90))
        row(c + "-R", 150, "45M20S", rand_seq(rng, 65))
        c, _ = contig(97 + v, left=v, right=v)
        row(c, 0, "*", "L-R")
        row(c, 0, "*", "L-R")                                      # both
    # a marker of the other side is a row like any other
    c, _ = contig(410)
    row(c + "-L", 1, "1S5M", "R")
    row(c + "-R", 196, "5M1S", "L")
    # IDs whose byte order is not their numeric order: L (99 / 100), left (negative), idx (2 / 10) -- and contigs without rows
    for L, left in ((99, -1), (100, -10), (1000, 30000), (99, -2), (101, 5)):
        contig(L, left=left, right=-left)
    # an original of one base or none is dropped with its consensus and takes no index (:433, :513)
    c, _ = contig(1)
    row(c, 1, "90S30M", rand_seq(rng, 120))
    row(c, -28, "30M90S", rand_seq(rng, 120))
    contig(0)
    # a name that matches no contig (idx beyond the set; the fields of another contig), lines with 3 fields
    row(f"Contig_99_0_0_{len(cs) + 5}", 1, "10S50M", rand_seq(rng, 60))
    row("Contig_99_-1_-1_0-L", 1, "10S50M", rand_seq(rng, 60))
    row("unknown", 1, "10S50M", rand_seq(rng, 60))
    text = "".join(f"Contig_{L}_{l}_{r}_{i},{b}\n" for i, (L, l, r, b) in enumerate(cs))
    lines = ["\t".join(str(x) for x in r) for r in rows] + ["Contig_99_-1_-1_0\t1\t10S50M", "a\tb\t\t", ""]
    lines = [lines[i] for i in rng.permutation(len(lines))]
    lines.append("Contig_130_-1_-1_8\t5\t6S50M\tACGTACGTAC" + rand_seq(rng, 46) + "\tMORE\tFIELDS")    # more than 4 fields
    return text, lines


def run_case(name, max_k, contig_text, lines, facts):
    cons, strings, text = ref_pipeline(contig_text, lines, max_k)
    f = {}
    mcons = em.consensus_rows(em.split_rows(lines), f)
    assert cons == mcons, name + " consensus rows"
    mstr = em.extend(em.contigs_of_text(contig_text), mcons)
    assert strings == mstr, name + " spliced strings"
    assert text == em.tag(mstr, max_k) == em.run_text(contig_text, lines, max_k), name + " text"
    ids = [s.split(",")[0] for s in strings]
    num = sorted(ids, key=lambda s: [int(x) for x in s.split("_")[1:5]])
    f.update(lflag=any(s.startswith("L-l1-") for _, s in cons), rflag=any(s.startswith("R-r1-") for _, s in cons),
             order=ids != num, dropped=len(strings) - text.count("\n"))
    facts[name] = f
    return cons, strings, text


def main():
    rng = np.random.default_rng(20261019)
    out, names, facts = {}, [], {}
    cases = []
    z = np.load(os.path.join(HERE, "fixing2_vectors.npz"))
    for name, mk, per_end in FIX2_CASES:
        text = z[name + "/text"].tobytes().decode()
        rows = []
        for ident, bases in em.contigs_of_text(text):
            rows += end_rows(rng, ident, bases, per_end)
        lines = ["\t".join(str(x) for x in r) for r in rows]
        cases.append(("fix_" + name, mk, text, [lines[i] for i in rng.permutation(len(lines))]))
    for mk in (31, 50):
        text, lines = crafted(rng, mk)
        cases.append((f"crafted_k{mk}", mk, text, lines))
    cases.append(("no_rows_k31", 31, cases[-1][2], []))
    cases.append(("empty_k31", 31, "", ["unknown\t1\t10S50M\t" + "ACGT" * 15]))
    for name, mk, text, lines in cases:
        cons, strings, final = run_case(name, mk, text, lines, facts)
        out[name + "/max_k"] = np.array([mk], np.int64)
        if not name.startswith("fix_"):
            out[name + "/contigs"] = np.frombuffer(text.encode(), np.uint8)
        out[name + "/rows"] = np.frombuffer("".join(r + "\n" for r in lines).encode(), np.uint8)
        out[name + "/cons"] = np.frombuffer("".join(f"{a}\t{b}\n" for a, b in cons).encode(), np.uint8)
        out[name + "/spliced"] = np.frombuffer("".join(s + "\n" for s in strings).encode(), np.uint8)
        out[name + "/text"] = np.frombuffer(final.encode(), np.uint8)
        names.append(name)
        print(name, text.count("\n"), "contigs", len(lines), "rows", len(final), "bytes of text", facts[name], flush=True)
    out["names"] = np.array(names)
    for what in ("lflag", "rflag", "tie", "cut", "order", "dropped"):
        if not any(f.get(what) for f in facts.values()):
            raise SystemExit(f"no case with {what}")
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "endext_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
