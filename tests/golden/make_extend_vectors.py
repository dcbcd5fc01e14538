#!/usr/bin/env python3
"""Golden vectors for the contig extension stages (Assembly_intermediate/08Extend, 09ExtendAgain) made by the REFERENCE'S OWN classes.

08Extend: the ten operator classes of P/ReflexivDSDynamicKmerExtend.java that its driver (`assemblyFromKmer`, :125-254) runs are
translated mechanically (tools/java2py.py, from the reference's source text at generation time) and driven in the driver's order, as
make_fixing_vectors.py drives the ten of the fixing stage: DynamicKmerBinarizerFromReducedToSubKmer ->
DSExtractFixingKmerFromContigEnds -> DSgetFixingLongKmer / DSgetFixingKmer -> groupBy("kmer").count() ->
DSFixingKmerLeftAndRightMarkerAssignment -> union -> sort("k-1") -> DSFilterForkSubKmerWithErrorCorrection ->
DSChangingFixingKmerToReflectedKmer -> sort("k-1") -> DSFilterForkReflectedSubKmerWithErrorCorrection -> DSExtendFixingKmerLoop (on
the fold's partitions, no sort) -> [sort("k-1") -> DSExtendFixingKmerLoop] x min(maximumIteration + 1, 17) ->
DSBinaryFixingKmerWithLongExtensionToString.  09ExtendAgain: the four classes of P/ReflexivDSDynamicKmerExtendRoundTwo.java (driver
:125-221) on the text of 08Extend, as make_fixing2_vectors.py drives its five: DynamicKmerBinarizerFromReducedToSubKmer -> [sort("k-1")
-> DSExtendFixingKmerLoop] x min(maximumIteration + 1, 29) -> DSBinaryFixingKmerToFullKmer -> zipWithIndex -> TagRowContigRDDID.  What
sits between two classes is Spark's, here as there: every sort stable on the SIGNED key long, P logical partitions cut at floor(p*n/P)
moved forward past equal keys, a fresh operator instance per partition.  No reference code is stored.

As in make_fixing_vectors.py every case runs TWICE, with the distinct 31-mers in first-occurrence order and shuffled, and the generator
FAILS if a stage from the first fold on differs.  Every stage of every case is ALSO computed by the string model
(tests/extend_model.py: its two own steps, then tests/fixing_model.py and tests/fixing2_model.py unchanged) and must agree -- every loop
pass with pymodel.dyn_extend_pass, the model of the EXISTING dynamic-k pass -- and the device's view of the input (bases without the
literals, and flags) must give the same 31-mers and long records as the text.  The generator fails unless both flags occur, a window
overlaps a seam by 1, 2 and 3 characters on each side, the loop merges in at least three different passes of a case that runs three or
more, and every branch of both folds is taken.

Output: tests/golden/extend_vectors.npz -- per case the input rows, the stages of 08 as fixing_vectors.npz stores them, the text of
08, every round of 09 as fixing2_vectors.npz stores them (under x2_), and the text of 09."""
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
import extend_model as xm  # noqa: E402
from make_reference_vectors import make_param, drain, u64, partition_starts  # noqa: E402
from make_dedup_vectors import blocks_to_seq, rand_seq  # noqa: E402
from make_ksort_vectors import attr3, pack_strings  # noqa: E402
from make_fixing_vectors import key_of, rec3, seq_of, compare, MARK  # noqa: E402
from make_fixing2_vectors import Tuple2  # noqa: E402

REF = os.environ.get("RFX_REFERENCE", "/root/reference") + "/src/main/java/uni/bielefeld/cmg/reflexiv/pipeline/"
CLASSES = ["DynamicKmerBinarizerFromReducedToSubKmer", "DSExtractFixingKmerFromContigEnds", "DSgetFixingLongKmer", "DSgetFixingKmer",
           "DSFixingKmerLeftAndRightMarkerAssignment", "DSFilterForkSubKmerWithErrorCorrection", "DSChangingFixingKmerToReflectedKmer",
           "DSFilterForkReflectedSubKmerWithErrorCorrection", "DSExtendFixingKmerLoop", "DSBinaryFixingKmerWithLongExtensionToString"]
CLASSES2 = ["DynamicKmerBinarizerFromReducedToSubKmer", "DSExtendFixingKmerLoop", "DSBinaryFixingKmerToFullKmer", "TagRowContigRDDID"]
# (name, max_k, P, scramble, max_iteration, contigs of the genome, the crafted rows too, a 3,000-base contig)
CASES = (("k31_P1_s2_M150", 31, 1, 2, 150, 10, True, False), ("k32_P2_s3_M150", 32, 2, 3, 150, 14, False, False),
         ("k41_P7_s2_M3", 41, 7, 2, 3, 10, True, True), ("k99_P63_s2_M0", 99, 63, 2, 0, 4, False, False),
         ("k31_P63_s3_M3", 31, 63, 3, 3, 6, False, False), ("k99_P2_s2_M3", 99, 2, 2, 3, 4, False, True))
_cls, _cls2 = {}, {}


def op(name, param):
    if not _cls:
        _cls.update(jp.translate_classes(REF + "ReflexivDSDynamicKmerExtend.java", CLASSES))
    return _cls[name](jp.Outer(param, _cls))


def op2(name, param):
    if not _cls2:
        _cls2.update(jp.translate_classes(REF + "ReflexivDSDynamicKmerExtendRoundTwo.java", CLASSES2))
    return _cls2[name](jp.Outer(param, _cls2))


def ref_param(p):
    param = make_param(31, maximumIteration=p["max_iteration"], scramble=p["scramble"])
    param.maxKmerSize = jp._I(p["max_k"])
    return param


def rec_bin(row):
    m, l, r = attr3(row.vals[1].v)
    _, ll, rl = attr3(row.vals[3].v)
    return seq_of(row.vals[0]), m, seq_of(row.vals[2]), l, r, ll, rl


def ref_pipeline(rows, p, P, shuffle=None):
    """-> ({stage: records}, {stage: partition starts}, {sort stage: permutation}, the 31-mers in emission order, the distinct
    31-mers' first occurrences, [loop passes], text)"""
    param = ref_param(p)
    st, ps, perms = {}, {}, {}
    one = lambda name, rs: drain(op(name, param).call(jp.JIter(rs)))                          # noqa: E731

    def parts(name, rs, tag_in, tag_out, starts=None):
        cuts = starts if starts is not None else partition_starts([key_of(r) for r in rs], P)
        out, ost = [], [0]
        for q in range(P):
            out += drain(op(name, param).call(jp.JIter(rs[cuts[q]:cuts[q + 1]])))
            ost.append(len(out))
        if tag_in:
            ps[tag_in], ps[tag_out] = cuts, ost
        return out, ost

    def sort(rs, name):
        perm = sorted(range(len(rs)), key=lambda i: key_of(rs[i]))                         # stable; signed
        if name:
            perms[name] = perm
        return [rs[i] for i in perm]

    cur = one("DynamicKmerBinarizerFromReducedToSubKmer", [jp.Row(r.rstrip("\n").split(",")) for r in rows])
    st["binarized"] = [rec_bin(r) for r in cur]
    full = one("DSExtractFixingKmerFromContigEnds", cur)
    longs = one("DSgetFixingLongKmer", full)
    st["long"] = [rec3(r) for r in longs]
    km = one("DSgetFixingKmer", full)
    kmers = [blocks_to_seq((u64(r.vals[0].v),)) for r in km]
    first = {}
    for i, r in enumerate(km):                                                               # groupBy("kmer").count()
        first.setdefault(u64(r.vals[0].v), i)
    order = list(first.values())
    if shuffle is not None:
        order = [order[i] for i in shuffle.permutation(len(order))]
    count = {}
    for r in km:
        count[u64(r.vals[0].v)] = count.get(u64(r.vals[0].v), 0) + 1
    counted = [jp.Row([km[i].vals[0], jp._L(count[u64(km[i].vals[0].v)])]) for i in order]
    cur = one("DSFixingKmerLeftAndRightMarkerAssignment", counted) + longs                   # union: the 31-mer records first
    st["union"] = [rec3(r) for r in cur]
    cur = sort(cur, "sort1")
    st["sort1"] = [rec3(r) for r in cur]
    cur, _ = parts("DSFilterForkSubKmerWithErrorCorrection", cur, "sort1", "fold1")
    st["fold1"] = [rec3(r) for r in cur]
    cur = one("DSChangingFixingKmerToReflectedKmer", cur)
    st["reflected"] = [rec3(r) for r in cur]
    cur = sort(cur, "sort2")
    st["sort2"] = [rec3(r) for r in cur]
    cur, ost = parts("DSFilterForkReflectedSubKmerWithErrorCorrection", cur, "sort2", "fold2")
    st["fold2"] = [rec3(r) for r in cur]
    cur, _ = parts("DSExtendFixingKmerLoop", cur, None, None, starts=ost)                    # the fold's partitions, no sort
    passes = [[rec3(r) for r in cur]]
    for _ in range(xm.loop_rounds(p)):
        cur = sort(cur, None)
        cur, _ = parts("DSExtendFixingKmerLoop", cur, None, None)
        passes.append([rec3(r) for r in cur])
    text = drain(op("DSBinaryFixingKmerWithLongExtensionToString", param).call(jp.JIter(cur)))
    return st, ps, perms, kmers, order, passes, "".join(f"{r.vals[0]},{r.vals[1]},{r.vals[2]}\n" for r in text)


def ref_pipeline2(rows, p, P):
    """the driver of 09ExtendAgain on the rows of 08Extend -> (the binarized records, [(sort permutation, output partition starts,
    records)] per round, the text)"""
    param = ref_param(p)
    cur = drain(op2("DynamicKmerBinarizerFromReducedToSubKmer", param).call(jp.JIter([jp.Row(r.rstrip("\n").split(",")) for r in rows])))
    binarized = [rec3(r) for r in cur]
    passes, ost = [], [0, len(cur)]
    iterations = 0
    while iterations <= p["max_iteration"]:                        # the driver's loop, :190-199
        iterations += 1
        if iterations >= 30:
            break
        perm = sorted(range(len(cur)), key=lambda i: key_of(cur[i]))                      # stable; signed
        cur = [cur[i] for i in perm]
        cuts = partition_starts([key_of(r) for r in cur], P)
        out, ost = [], [0]
        for q in range(P):
            out += drain(op2("DSExtendFixingKmerLoop", param).call(jp.JIter(cur[cuts[q]:cuts[q + 1]])))
            ost.append(len(out))
        cur = out
        passes.append((perm, ost, [rec3(r) for r in cur]))
    full = []
    for q in range(len(ost) - 1):
        full += drain(op2("DSBinaryFixingKmerToFullKmer", param).call(jp.JIter(cur[ost[q]:ost[q + 1]])))
    tagged = []
    for idx, s in enumerate(full):                                 # zipWithIndex: over the partitions in order
        tagged += drain(op2("TagRowContigRDDID", param).call(Tuple2(s, jp._L(idx))))
    return binarized, passes, "".join(f"{r.vals[0]},{r.vals[1]}\n" for r in tagged)


def end_row(rows, idx, left_end, contig, right_end, left, right, fl=False, fr=False):
    """a row of 07EndExtend as its writer writes it: the literals behind the left end and ahead of the right one where flagged"""
    lt, rt = left_end + ("-1l" if fl else ""), ("r1-" if fr else "") + right_end
    rows.append(f">Contig_{len(contig)}_{left}_{right}_{idx}_{len(lt)}_{len(rt)}_{len(rows)},{lt}{contig}{rt}")


def make_rows(rng, mk, n_contigs, crafted, big):
    """07EndExtend texts: contigs cut from a small genome, each with the consensus ends that reach into its neighbours, so that the end
    31-mers of neighbours meet and the loop joins the cut contigs; + the crafted rows of the issue"""
    rows = []
    g = rand_seq(rng, 260 * n_contigs + 900)
    pos = 320
    for c in range(n_contigs):
        L = int(rng.integers(2 * mk + 10, 2 * mk + 120))
        ll, rl = int(rng.integers(0, 70)), int(rng.integers(0, 70))
        fl, fr = bool(rng.integers(0, 4) == 0), bool(rng.integers(0, 4) == 0)
        # (a flagged seam breaks the chain of 31-mers there: three T stand between the end and the contig)
        end_row(rows, c, g[pos - ll:pos], g[pos:pos + L], g[pos + L:pos + L + rl], int(rng.choice(MARK)), int(rng.choice(MARK)), fl, fr)
        pos += L + int(rng.integers(-25, 45))
    if not crafted:
        return rows
    n = [len(rows)]

    def row(L, ll, rl, left=None, right=None, fl=False, fr=False, contig=None, le=None, re=None):
        left = int(rng.choice(MARK)) if left is None else left
        right = int(rng.choice(MARK)) if right is None else right
        end_row(rows, n[0], rand_seq(rng, ll) if le is None else le, contig or rand_seq(rng, L), rand_seq(rng, rl) if re is None else re,
                left, right, fl, fr)
        n[0] += 1

    base = 2 * mk + 20
    full = (300,) if mk == 31 else ()                              # (ends of 300 bases make 300 records each: in one case only)
    for e in (0, 1, 2, 4, 30, 31, 32, 33) + full:                   # ll and rl each of 0, 1, 2, 4, 30..33, 300 (unflagged)
        row(base, e, int(rng.integers(0, 40)))
        row(base, int(rng.integers(0, 40)), e)
    for fl, fr in ((False, False), (True, False), (False, True), (True, True)):              # all four flag patterns
        for e in (0, 1, 27, 28, 29, 30, 31) + full:                  # a flag alone (3), 4, 30..34, 303: the seam at every edge of a window
            row(base + e, e, e, fl=fl, fr=fr)
    if full:
        row(base, 300, 300, fl=True, fr=True)                      # 303 + 303 = 606 end 31-mers of one contig
    for L in (32, 33, 61, 62, 63, 64, 65):                         # cut lengths on the key's and the words' edges
        row(L, mk, mk, fl=bool(L & 1), fr=bool(L & 2))
    for left, right in ((-5, 0), (0, 1), (1, 2), (2, 7), (30000, -30000), (30001, -30001), (-30001, 30001)):
        row(base + 9, 12, 13, left=left, right=right)
    d = rand_seq(rng, base + 30)                                   # a contig and its duplicate
    row(0, 20, 20, contig=d, left=-1, right=-1)
    row(0, 20, 20, contig=d, left=3, right=-1)
    e = rand_seq(rng, 31)                                          # two contigs sharing an end 31-mer
    row(base, 5, 0, le=e[:5], contig=e[5:] + rand_seq(rng, base))
    row(base, 9, 0, le=e[:9], contig=e[9:] + rand_seq(rng, base))
    v = rand_seq(rng, base + 40)                                   # an end 31-mer on a cut contig's key: u's right end runs into v's start
    u = rand_seq(rng, base)
    row(0, 10, 40, contig=u, re=v[:40])
    row(0, 10, 10, contig=v)
    row(0, 10, 40, contig=rand_seq(rng, base), re=v[len(v) - 35:] + rand_seq(rng, 5))        # ... and into v's end
    for tot in (2 * mk - 1, 2 * mk):                               # a row one character below 2 max_k, and one at it
        row(tot - 20, 10, 10)
    end_row(rows, -7, rand_seq(rng, 8), rand_seq(rng, base), rand_seq(rng, 8), -3, -4)       # IDs with negative fields
    rows[-1] = rows[-1].replace(f"_{len(rows) - 1},", "_-9,")
    s = rand_seq(rng, base + 30)
    end_row(rows, n[0], "ACGNT", s[:40] + "N" + s[41:70] + "n" + s[71:], "xACG", 2, 2)           # letters that are not ACGT read as T
    if big:
        row(3000 + int(rng.integers(0, 64)), 300, 17, fl=True)
        row(3100 + int(rng.integers(0, 64)), 3, 300, fr=True)
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


def run_case(name, p, P, rows, hits, rng):
    st, ps, perms, kmers, order, passes, text = ref_pipeline(rows, p, P)
    st2, ps2, _, kmers2, _, passes2, text2 = ref_pipeline(rows, p, P, shuffle=rng)
    assert kmers2 == kmers and sorted(st2["union"]) == sorted(st["union"]) and st2["union"] != st["union"], name + ": the shuffled run"
    for s in ("fold1", "reflected", "sort2", "fold2"):             # the proof that the order contract does not need groupBy's order
        assert st2[s] == st[s] and ps2.get(s) == ps.get(s), f"{name}: stage {s} depends on the order of the distinct 31-mers"
    assert passes2 == passes and text2 == text, name + ": the loop depends on the order of the distinct 31-mers"
    mst, mps, mk, mpasses = xm.run_stages(rows, p, P, hits)
    compare(kmers, mk, name + " 31-mers")
    for s in xm.STAGES:
        compare(st[s], mst[s], f"{name} {s}")
        if s in ps:
            compare(ps[s], mps[s], f"{name} {s} partition starts")
    assert len(passes) == len(mpasses) == 1 + xm.loop_rounds(p)
    for i, (a, b) in enumerate(zip(passes, mpasses)):              # the loop IS the dynamic-k pass: every loop stage agrees
        compare(a, b, f"{name} loop pass {i}")
    assert text == xm.to_text(mpasses[-1]), name + " text"
    for q in range(P):                                             # the closed form of both folds
        for a, b in (("sort1", "fold1"), ("sort2", "fold2")):
            assert fm.fold_closed_form(st[a][ps[a][q]:ps[a][q + 1]]) == st[b][ps[b][q]:ps[b][q + 1]], f"{name}: closed form of {b}"
    # the device's view of the same rows: the literals in flags / as T bases
    for in_flags in (True, False):
        dl, dk = xm.set_contig_ends(xm.device_set(rows, p, in_flags), p)
        assert (dl, dk) == (st["long"], kmers), f"{name}: the device's view (literals in flags: {in_flags})"
    merging = sum(1 for a, b in zip([st["fold2"]] + passes, passes) if len(b) < len(a))
    # 09ExtendAgain on the text of 08
    rows2 = text.splitlines()
    binarized, rounds2, text2 = ref_pipeline2(rows2, p, P)
    mrecs = f2.binarize(rows2)
    compare(binarized, mrecs, name + " 09 binarized")
    mrounds = f2.run_passes(mrecs, p, P, hits)
    assert len(rounds2) == len(mrounds) == f2.loop_rounds(p), name
    for i, (a, b) in enumerate(zip(rounds2, mrounds)):
        assert a[0] == b[0] and a[1] == b[1], f"{name} 09 sort / partition starts {i}"
        compare(a[2], b[2], f"{name} 09 pass {i}")
    assert text2 == xm.to_text2(f2.contigs(rounds2[-1][2] if rounds2 else binarized, p)) == xm.run2_text(rows2, p, P), name + " 09 text"
    return (st, ps, perms, kmers, order, passes, text, binarized, rounds2, text2), merging


def put_pass(out, tag, srt, recs):
    """a loop pass as fixing2_vectors.npz stores one: a record that the loop only passed on or flipped as the index of its source in
    the pass's input and its marker, a merged record in full"""
    src, fresh = f2.pass_sources(srt, recs)
    assert f2.pass_from_sources(srt, src, [r[1] for r in recs], fresh) == recs
    out[tag + "_src"] = np.array(src, np.int32)
    out[tag + "_marker"] = np.array([r[1] for r in recs], np.int8)
    out[tag + "_key"], out[tag + "_key_off"] = pack_strings([r[0] for r in fresh])
    out[tag + "_ext"], out[tag + "_ext_off"] = pack_strings([r[2] for r in fresh])
    out[tag + "_lr"] = np.array([(r[3], r[4]) for r in fresh], np.int32).reshape(-1, 2)
    assert xm.get_pass(out, tag, srt) == recs


def store(out, name, p, P, rows, res):
    st, ps, perms, kmers, order, passes, text, binarized2, rounds2, text2 = res
    out[name + "/meta"] = np.array([p["max_k"], p["scramble"], p["max_iteration"], P, len(passes), len(rounds2)], np.int64)
    out[name + "/rows"], out[name + "/rows_off"] = pack_strings([r + "\n" for r in rows])
    out[name + "/kmers"], out[name + "/kmers_off"] = pack_strings(kmers)

    def records(tag, recs):
        out[f"{name}/{tag}_key"], out[f"{name}/{tag}_key_off"] = pack_strings([r[0] for r in recs])
        out[f"{name}/{tag}_ext"], out[f"{name}/{tag}_ext_off"] = pack_strings([r[2] for r in recs])
        out[f"{name}/{tag}_mlr"] = np.array([(r[1], r[3], r[4]) for r in recs], np.int32).reshape(-1, 3)

    assert st["binarized"] == xm.binarize(rows, p)                 # (the rows ARE the binarizer's output)
    records("long", st["long"])
    assert [fm.kmer_set([kmers[i]], [])[0] for i in order] + st["long"] == st["union"]
    out[name + "/union_kmers"] = np.array(order, np.int32)
    prev = st["union"]
    for s in ("sort1", "fold1", "reflected", "sort2", "fold2"):
        recs = st[s]
        if s in ps:
            out[f"{name}/{s}_ps"] = np.array(ps[s], np.int64)
        if s in perms:
            out[f"{name}/{s}_perm"] = np.array(perms[s], np.int32)
        elif s.startswith("fold"):                                 # every output row is an input row, in order
            src, j = [], 0
            for r in recs:
                while prev[j] != r:
                    j += 1
                src.append(j)
                j += 1
            out[f"{name}/{s}_from"] = np.array(src, np.int32)
        else:                                                      # the reflection: every record is its input's, flipped to marker 2
            put_pass(out, f"{name}/{s}", prev, recs)
            assert not len(out[f"{name}/{s}_lr"])
        prev = recs
    prev = st["fold2"]
    for i, recs in enumerate(passes[:-1]):                         # (the last pass IS the text; the first runs on the fold's order)
        put_pass(out, f"{name}/pass{i}", prev if i == 0 else fm.sort_records(prev), recs)
        prev = recs
    assert fm.from_text(text) == passes[-1]
    out[name + "/text"] = np.frombuffer(text.encode(), np.uint8)
    prev = binarized2
    for i, (perm, ost, recs) in enumerate(rounds2):
        tag = f"{name}/x2_"
        out[f"{tag}sort{i}_perm"] = np.array(perm, np.int32)
        out[f"{tag}pass{i}_ps"] = np.array(ost, np.int64)
        put_pass(out, f"{tag}pass{i}", [prev[j] for j in perm], recs)
        prev = recs
    out[name + "/text2"] = np.frombuffer(text2.encode(), np.uint8)


def main():
    rng = np.random.default_rng(20261022)
    out, names, hits = {}, [], {}
    overlaps, flags_seen = set(), set()
    for name, mk, P, scramble, max_it, n_contigs, crafted, big in CASES:
        p = xm.default_params(mk, scramble=scramble, max_iteration=max_it)
        rows = make_rows(rng, mk, n_contigs, crafted, big)
        res, merging = run_case(name, p, P, rows, hits, rng)
        store(out, name, p, P, rows, res)
        names.append(name)
        dev = xm.device_set(rows, p)
        overlaps |= xm.seam_overlaps(dev, p)
        flags_seen |= {c["flags"] for c in dev}
        st, passes = res[0], res[5]
        print(name, len(rows), "rows ->", {s: len(st[s]) for s in xm.STAGES}, "passes", [len(x) for x in passes], "merging passes", merging,
              "09 rounds", [len(x[2]) for x in res[8]][:6], "contigs", res[9].count("\n"), flush=True)
        if len(passes) >= 3 and merging < 3 and (crafted or P < 63):
            raise SystemExit(f"{name}: the loop merges in {merging} passes only")
    out["names"] = np.array(names)
    if flags_seen != {0, 1, 2, 3}:
        raise SystemExit(f"flag patterns {sorted(flags_seen)} only")
    want = {(s, n) for s in "LR" for n in (1, 2, 3)}
    if overlaps != want:
        raise SystemExit(f"seam overlaps never taken: {sorted(want - overlaps)}")
    every = [f"{t} {b}" for t in "LR" for b in fm.FOLD_BRANCHES if (t, b) != ("L", "short_after_long_dropped")] + list(fm.LOOP_BRANCHES)
    print("branch hits", {b: hits.get(b, 0) for b in every}, flush=True)
    missing = [b for b in every if not hits.get(b) and b[:2] in ("L ", "R ")]    # (the folds' branches; the loop's are fixing_vectors.npz's to cover)
    if missing and "--allow-missing" not in sys.argv:
        raise SystemExit(f"branches never taken: {missing}")
    out["branch_names"] = np.array(every)
    out["branch_hits"] = np.array([hits.get(b, 0) for b in every], np.int64)
    assert {c[1] for c in CASES} == {31, 32, 41, 99} and {c[2] for c in CASES} == {1, 2, 7, 63}
    assert {c[3] for c in CASES} == {2, 3} and {c[4] for c in CASES} == {0, 3, 150}
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "extend_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
