#!/usr/bin/env python3
"""Golden vectors for the second contig fixing stage (Assembly_intermediate/05FixingAgain, 06ContigEnds) made by the REFERENCE'S
OWN classes.

The five classes of P/ReflexivDSDynamicKmerFixingRoundTwo.java that its driver (`assemblyFromKmer`, :138-263) runs are
translated mechanically (tools/java2py.py, from the reference's source text at generation time) and driven in the driver's
order: DynamicKmerBinarizerFromReducedToSubKmer -> [sort("k-1") -> DSExtendFixingKmerLoop] x min(maximumIteration + 1, 29) ->
DSBinaryFixingKmerWithLongExtensionToString -> zipWithIndex -> TagStringContigRDDID -> DSExtractContigEndsForAlignment.  What
sits between two classes is Spark's, here as in make_fixing_vectors.py: every sort stable on the SIGNED key long, P logical
partitions cut at floor(p*n/P) moved forward past equal keys, a fresh operator instance per partition, zipWithIndex running
over the partitions in order.  No reference code is stored.

Every pass of every case is ALSO computed by the string model (tests/fixing2_model.py -- its loop is fixing_model.loop_pass,
which wraps pymodel.dyn_extend_pass, the model of the EXISTING dynamic-k pass) and must agree in records and partition starts;
the model refuses a branch of that pass that the fixing loop cannot reach.  So do both texts.

Inputs: the final text of the nine cases of fixing_vectors.npz under their own parameters, and new sets -- fixing_model.run_text
at max_iteration 0 and 3 on overlapping contigs, so that this stage's loop has work left, plus crafted rows in the form of
04Fixing.  The generator FAILS unless at least three cases merge in at least three different rounds, both branches of the 400
rule and of the length filter are taken, and a dropped contig precedes a kept one.

Output: tests/golden/fixing2_vectors.npz -- per case the input rows (a case named fix_<name> has none: its rows are the text of case
<name> of fixing_vectors.npz), per round the sort as the permutation of the set before it,
the loop's output partition starts and the records behind it (a record that the loop only passed on or flipped as the index of its
source in the sorted set and its marker, a merged record in full), and both texts."""
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
import fixing_model as fm  # noqa: E402
import fixing2_model as f2  # noqa: E402
from make_reference_vectors import make_param, drain, partition_starts  # noqa: E402
from make_dedup_vectors import rand_seq  # noqa: E402
from make_ksort_vectors import pack_strings  # noqa: E402
from make_fixing_vectors import key_of, rec3, make_rows, compare  # noqa: E402

REF = os.environ.get("RFX_REFERENCE", "/root/reference") + "/src/main/java/uni/bielefeld/cmg/reflexiv/pipeline/"
CLASSES = ["DynamicKmerBinarizerFromReducedToSubKmer", "DSExtendFixingKmerLoop", "DSBinaryFixingKmerWithLongExtensionToString",
           "TagStringContigRDDID", "DSExtractContigEndsForAlignment"]
# new inputs: (name, max_k, P, scramble, max_iteration, the first stage's max_iteration, contigs of the genome, a 3,000-base contig)
NEW_CASES = (("new_k31_P2_s2_M-1", 31, 2, 2, -1, 0, 10, False), ("new_k41_P7_s3_M27", 41, 7, 3, 27, 3, 12, False),
             ("new_k32_P1_s2_M28", 32, 1, 2, 28, 0, 10, False), ("new_k99_P63_s2_M3", 99, 63, 2, 3, 0, 4, True),
             ("new_k31_P7_s3_M150", 31, 7, 3, 150, 3, 12, True))
_cls = {}


class Tuple2:
    """scala.Tuple2, as far as TagStringContigRDDID reads it"""

    def __init__(self, a, b):
        self.a, self.b = a, b

    def _1(self):
        return self.a

    def _2(self):
        return self.b


def op(name, param):
    if not _cls:
        _cls.update(jp.translate_classes(REF + "ReflexivDSDynamicKmerFixingRoundTwo.java", CLASSES))
    return _cls[name](jp.Outer(param, _cls))


def ref_param(p):
    param = make_param(31, maximumIteration=p["max_iteration"], scramble=p["scramble"])
    param.maxKmerSize = jp._I(p["max_k"])
    return param


def ref_pipeline(rows, p, P):
    """-> (the binarized records, [(sort permutation, output partition starts, records)] per round, 05FixingAgain, 06ContigEnds)"""
    param = ref_param(p)
    cur = drain(op("DynamicKmerBinarizerFromReducedToSubKmer", param).call(jp.JIter([jp.Row(r.rstrip("\n").split(",")) for r in rows])))
    binarized = [rec3(r) for r in cur]
    passes, ost = [], [0, len(cur)]
    iterations = 0
    while iterations <= p["max_iteration"]:                        # the driver's loop, :203-213
        iterations += 1
        if iterations >= 30:
            break
        perm = sorted(range(len(cur)), key=lambda i: key_of(cur[i]))                      # stable; signed
        cur = [cur[i] for i in perm]
        cuts = partition_starts([key_of(r) for r in cur], P)
        out, ost = [], [0]
        for q in range(P):
            out += drain(op("DSExtendFixingKmerLoop", param).call(jp.JIter(cur[cuts[q]:cuts[q + 1]])))
            ost.append(len(out))
        cur = out
        passes.append((perm, ost, [rec3(r) for r in cur]))
    strings = []
    for q in range(len(ost) - 1):
        strings += drain(op("DSBinaryFixingKmerWithLongExtensionToString", param).call(jp.JIter(cur[ost[q]:ost[q + 1]])))
    tagged = []
    for idx, s in enumerate(strings):                              # zipWithIndex: over the partitions in order
        tagged += drain(op("TagStringContigRDDID", param).call(Tuple2(s, jp._L(idx))))
    text = "".join(f"{r.vals[0]},{r.vals[1]}\n" for r in tagged)
    ends = "".join(s + "\n" for s in drain(op("DSExtractContigEndsForAlignment", param).call(jp.JIter(tagged))))
    return binarized, passes, text, ends


def crafted_rows(rng, mk, big):
    """rows in the form of 04Fixing (30-base keys): contig lengths on the filter's edge and on the 400 rule's, both markers, short
    extensions, every sign of left / right, tuple text"""
    rows = []

    def row(L, marker, left=-1, right=-1, tuple_text=False):
        c = rand_seq(rng, L)
        key, ext = (c[:30], c[30:]) if marker == 1 else (c[L - 30:], c[:L - 30])
        rows.append(f"({key},{marker}|{left}|{right}),{ext}" if tuple_text else f"{key},{marker}|{left}|{right},{ext}")

    for L in (2 * mk - 1, 2 * mk, 2 * mk + 1, 399, 400, 401):
        for m in (1, 2):
            row(L, m, left=int(rng.choice((-1, 0, 7))), right=int(rng.choice((-1, 0, 7))))
    for e in (1, 2, 31, 32, 33, 34, 63, 64, 65):
        row(30 + e, 1 + e % 2)
    for left in (-5, 0, 5, 30000, -30000):
        for right in (-5, 0, 5, 30000, -30000):
            row(2 * mk + 3 + int(rng.integers(0, 40)), 1 + (left + right) % 2, left=left, right=right)
    row(2 * mk + 50, 1, tuple_text=True)
    row(2 * mk + 50, 2, left=3, right=-2, tuple_text=True)
    if big:
        row(3000 + int(rng.integers(0, 64)), 1, left=-1, right=12)
        row(3100 + int(rng.integers(0, 64)), 2, left=12, right=-1)
    return rows


def run_case(name, p, P, rows, hits):
    binarized, passes, text, ends = ref_pipeline(rows, p, P)
    mrecs = f2.binarize(rows)
    compare(binarized, mrecs, name + " binarized")
    mpasses = f2.run_passes(mrecs, p, P, hits)                     # (raises where the loop takes a branch the dynamic-k pass's model refuses)
    assert len(passes) == len(mpasses) == f2.loop_rounds(p), name
    for i, (a, b) in enumerate(zip(passes, mpasses)):              # the loop IS the existing pass: every round agrees
        assert a[0] == b[0], f"{name} sort {i}"
        assert a[1] == b[1], f"{name} partition starts behind pass {i}"
        compare(a[2], b[2], f"{name} pass {i}")
    last = passes[-1][2] if passes else binarized
    cs = f2.contigs(last, p)
    assert text == f2.to_text(cs), name + " text"
    assert ends == f2.ends_text(cs), name + " ends"
    sizes = [len(binarized)] + [len(x[2]) for x in passes]
    merging = sum(1 for a, b in zip(sizes, sizes[1:]) if b < a)
    kept = [len(fm.contig_of(r)) >= 2 * p["max_k"] for r in last]
    facts = dict(merging=merging, dropped=kept.count(False), kept=kept.count(True),
                 dropped_before_kept=any(not a and any(kept[i + 1:]) for i, a in enumerate(kept)),
                 two_ends=sum(1 for c in cs if len(c[0]) >= 400), one_end=sum(1 for c in cs if len(c[0]) < 400))
    return (binarized, passes, text, ends), facts


def store(out, name, p, P, rows, res):
    binarized, passes, text, ends = res
    out[name + "/meta"] = np.array([p["max_k"], p["scramble"], p["max_iteration"], P, len(passes)], np.int64)
    if not name.startswith("fix_"):                                # (a fix_ case reads the text of its case of fixing_vectors.npz)
        out[name + "/rows"], out[name + "/rows_off"] = pack_strings([r + "\n" for r in rows])
    prev = binarized
    for i, (perm, ost, recs) in enumerate(passes):
        out[f"{name}/sort{i}_perm"] = np.array(perm, np.int32)
        out[f"{name}/pass{i}_ps"] = np.array(ost, np.int64)
        srt = [prev[j] for j in perm]
        src, fresh = f2.pass_sources(srt, recs)                   # a row the loop only flipped is stored as its source and its marker
        assert f2.pass_from_sources(srt, src, [r[1] for r in recs], fresh) == recs
        out[f"{name}/pass{i}_src"] = np.array(src, np.int32)
        out[f"{name}/pass{i}_marker"] = np.array([r[1] for r in recs], np.int8)
        out[f"{name}/pass{i}_key"], out[f"{name}/pass{i}_key_off"] = pack_strings([r[0] for r in fresh])
        out[f"{name}/pass{i}_ext"], out[f"{name}/pass{i}_ext_off"] = pack_strings([r[2] for r in fresh])
        out[f"{name}/pass{i}_lr"] = np.array([(r[3], r[4]) for r in fresh], np.int32).reshape(-1, 2)
        prev = recs
    out[name + "/text"] = np.frombuffer(text.encode(), np.uint8)
    out[name + "/ends"] = np.frombuffer(ends.encode(), np.uint8)


def main():
    rng = np.random.default_rng(20261021)
    out, names, hits, facts = {}, [], {}, {}
    cases = []
    z = np.load(os.path.join(HERE, "fixing_vectors.npz"))
    for name in [str(x) for x in z["names"]]:                      # the nine stored fixing outputs, under their own parameters
        v = z[name + "/meta"]
        p = f2.default_params(int(v[0]), scramble=int(v[1]), max_iteration=int(v[2]))
        cases.append(("fix_" + name, p, int(v[3]), z[name + "/text"].tobytes().decode().splitlines()))
    for name, mk, P, scramble, max_it, first_it, n_contigs, big in NEW_CASES:
        p1 = fm.default_params(mk, scramble=scramble, max_iteration=first_it)
        rows = fm.run_text(make_rows(rng, mk, n_contigs, False, False), p1, P).splitlines() + crafted_rows(rng, mk, big)
        rows = [rows[i] for i in rng.permutation(len(rows))]
        cases.append((name, f2.default_params(mk, scramble=scramble, max_iteration=max_it), P, rows))
    for name, p, P, rows in cases:
        res, facts[name] = run_case(name, p, P, rows, hits)
        store(out, name, p, P, rows, res)
        names.append(name)
        print(name, len(rows), "rows, rounds", len(res[1]), "sizes", [len(x[2]) for x in res[1]][:6], facts[name], flush=True)
    out["names"] = np.array(names)
    three = [n for n, f in facts.items() if f["merging"] >= 3]
    if len(three) < 3:
        raise SystemExit(f"only {three} merge in three different rounds or more")
    for what in ("dropped", "kept", "two_ends", "one_end"):
        if not any(f[what] for f in facts.values()):
            raise SystemExit(f"no case with {what}")
    if not any(f["dropped_before_kept"] for f in facts.values()):
        raise SystemExit("no case where a dropped contig precedes a kept one")
    assert {p["max_k"] for _, p, _, _ in cases} == {31, 32, 41, 99} and {P for _, _, P, _ in cases} == {1, 2, 7, 63}
    assert {p["scramble"] for _, p, _, _ in cases} == {2, 3} and {p["max_iteration"] for _, p, _, _ in cases} == {-1, 0, 3, 27, 28, 150}
    out["merging_rounds"] = np.array([facts[n]["merging"] for n in names], np.int64)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "fixing2_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
