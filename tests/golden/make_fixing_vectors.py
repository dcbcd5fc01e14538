#!/usr/bin/env python3
"""Golden vectors for the contig fixing stage (Assembly_intermediate/04Fixing) made by the REFERENCE'S OWN classes.

The ten operator classes of P/ReflexivDSDynamicKmerFixing.java that its driver (`assemblyFromKmer`, :125-260) runs are
translated mechanically (tools/java2py.py, from the reference's source text at generation time) and driven in the driver's
order: DynamicKmerBinarizerFromReducedToSubKmer -> DSExtractFixingKmerFromContigEnds -> DSgetFixingLongKmer / DSgetFixingKmer ->
groupBy("kmer").count() -> DSFixingKmerLeftAndRightMarkerAssignment -> union (the 31-mer records first) -> sort("k-1") ->
DSFilterForkSubKmerWithErrorCorrection -> DSChangingFixingKmerToReflectedKmer -> sort("k-1") ->
DSFilterForkReflectedSubKmerWithErrorCorrection -> DSExtendFixingKmerLoop (on the fold's partitions, no sort) ->
[sort("k-1") -> DSExtendFixingKmerLoop] x min(maximumIteration + 1, 17) -> DSBinaryFixingKmerWithLongExtensionToString.
What sits between two classes is Spark's; here: every sort stable on the SIGNED key long, P logical partitions cut at
floor(p*n/P) moved forward past equal keys (make_reference_vectors.partition_starts), a fresh operator instance per
partition.  No reference code is stored.

groupBy's output order is Spark's hash order, which nobody reproduces.  Every case is therefore run TWICE, with the distinct
31-mers in first-occurrence order and shuffled by a seeded permutation, and the generator FAILS if a stage from the first
fold on differs: nothing behind the sort depends on that order.  Only the first-occurrence run is stored.

Every stage of every case is ALSO computed by the string model (tests/fixing_model.py) and must agree -- the loop's stages
with pymodel.dyn_extend_pass, the model of the EXISTING dynamic-k pass: the vectors decide that step 9 is that pass.  The
model counts the branches of both folds and of the loop; the generator fails if one is never taken, and if the loop merges
in fewer than three different passes of a case.

Output: tests/golden/fixing_vectors.npz -- per case the input rows, the record set behind every stage (the binarizer's as the
kept rows' indices, the union's 31-mer records as indices into the 31-mers in emission order, a sort as the permutation of
the stage before it, a fold as indices into its input), the partition starts in and out of the folds, every loop pass (the last one as
the text), and the text."""
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
from make_reference_vectors import make_param, drain, u64, partition_starts  # noqa: E402
from make_dedup_vectors import blocks_of, blocks_to_seq, rand_seq  # noqa: E402
from make_ksort_vectors import attr3, pack_strings  # noqa: E402

REF = os.environ.get("RFX_REFERENCE", "/root/reference") + "/src/main/java/uni/bielefeld/cmg/reflexiv/pipeline/"
CLASSES = ["DynamicKmerBinarizerFromReducedToSubKmer", "DSExtractFixingKmerFromContigEnds", "DSgetFixingLongKmer", "DSgetFixingKmer",
           "DSFixingKmerLeftAndRightMarkerAssignment", "DSFilterForkSubKmerWithErrorCorrection", "DSChangingFixingKmerToReflectedKmer",
           "DSFilterForkReflectedSubKmerWithErrorCorrection", "DSExtendFixingKmerLoop", "DSBinaryFixingKmerWithLongExtensionToString"]
# (name, max_k, P, scramble, max_iteration, contigs of the genome, the crafted rows too, a 3,000-base contig)
CASES = (("k31_P1_s2_M150", 31, 1, 2, 150, 14, True, False), ("k32_P2_s3_M150", 32, 2, 3, 150, 14, True, False),
         ("k41_P7_s2_M3", 41, 7, 2, 3, 12, True, False), ("k99_P63_s2_M0", 99, 63, 2, 0, 3, True, True),
         ("k31_P63_s3_M150", 31, 63, 3, 150, 9, False, False), ("k41_P63_s2_M3", 41, 63, 2, 3, 2, False, False),
         ("k31_P7_s3_M0", 31, 7, 3, 0, 8, True, True), ("k99_P2_s2_M3", 99, 2, 2, 3, 4, False, False),
         ("k32_P1_s2_M3", 32, 1, 2, 3, 8, True, False))
_cls = {}


def op(name, param):
    if not _cls:
        _cls.update(jp.translate_classes(REF + "ReflexivDSDynamicKmerFixing.java", CLASSES))
    return _cls[name](jp.Outer(param, _cls))


def ref_param(p):
    param = make_param(31, maximumIteration=p["max_iteration"], scramble=p["scramble"])
    param.maxKmerSize = jp._I(p["max_k"])
    return param


def sgn(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def key_of(row):
    return sgn(row.vals[0].v)                                      # ONE long, compared signed


def seq_of(x):
    return blocks_to_seq(blocks_of(x))


def rec3(row):
    """(key long, attribute, extension blocks) -> the model's record"""
    m, l, r = attr3(row.vals[1].v)
    return blocks_to_seq((u64(row.vals[0].v),)), m, seq_of(row.vals[2]), l, r


def rec_bin(row):
    m, l, r = attr3(row.vals[1].v)
    return seq_of(row.vals[0]), m, seq_of(row.vals[2]), l, r


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
    full = one("DSExtractFixingKmerFromContigEnds", cur)                                     # (blocks, attribute)
    longs = one("DSgetFixingLongKmer", full)
    st["long"] = [rec3(r) for r in longs]
    km = one("DSgetFixingKmer", full)                                                        # (kmer long, 1)
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
    for _ in range(fm.loop_rounds(p)):
        cur = sort(cur, None)
        cur, _ = parts("DSExtendFixingKmerLoop", cur, None, None)
        passes.append([rec3(r) for r in cur])
    text = drain(op("DSBinaryFixingKmerWithLongExtensionToString", param).call(jp.JIter(cur)))
    return st, ps, perms, kmers, order, passes, "".join(f"{r.vals[0]},{r.vals[1]},{r.vals[2]}\n" for r in text)


MARK = (-30000, -7, -1, 0, 1, 2, 9, 30000)


def make_rows(rng, mk, n_contigs, crafted, big):
    """the rows of an Iteration output: contigs cut from a small random genome so that their ends overlap (the loop then
    merges them through the chain of end 31-mers) + the crafted rows of the issue"""
    rows = []
    cut = mk - 30

    def row(contig, marker=None, left=None, right=None, klen=None, tuple_text=False):
        marker = marker or int(rng.integers(1, 3))
        klen = klen or int(rng.choice((30, 31, 32, mk - 1, min(124, 2 * mk))))
        klen = min(klen, len(contig) - 1)
        left = int(rng.choice(MARK)) if left is None else left
        right = int(rng.choice(MARK)) if right is None else right
        key, ext = (contig[:klen], contig[klen:]) if marker == 1 else (contig[len(contig) - klen:], contig[:len(contig) - klen])
        rows.append(f"({key},{marker}|{left}|{right}),{ext}" if tuple_text else f"{key},{marker}|{left}|{right},{ext}")

    g = rand_seq(rng, 140 * n_contigs + 400)
    pos = 0
    for c in range(n_contigs):                                     # neighbours overlap by 31 .. 2 cut + 58 bases: their end chains meet
        L = int(rng.integers(2 * mk + 40, 2 * mk + 150))
        row(g[pos:pos + L])
        pos += L - int(rng.integers(31, 2 * cut + 59))
    if not crafted:
        return rows
    # pairs whose TRIMMED contigs share a 30-base key: A's last 30 bases are B's first 30 -- two long rows meet in the loop, under
    # every sign pattern of (A's right, B's left), as forward row / reflected holder and the other way round
    pairs = ((-1, -1), (5, 7), (30000, -3), (-3, 30000), (1, -1), (-1, 1), (0, -1), (-1, 0), (-9, -9), (2, 2), (40, -1), (-1, 40))
    for la, rb in pairs[:6 if mk >= 99 else 12]:                   # (max_k 99 makes 139 records of every row: half of them there)
        s = rand_seq(rng, 4 * mk + 200)
        b = 2 * mk + 60 + int(rng.integers(0, 30))
        row(s[:b], left=int(rng.choice(MARK)), right=la)
        row(s[b - 2 * cut - 30:], left=rb, right=int(rng.choice(MARK)))
    for L in (2 * mk - 1, 2 * mk, 2 * mk + 1):                     # the length filter's edge
        for m in (1, 2):
            row(rand_seq(rng, L), marker=m)
    for tot in (62, 63, 64, 65, 93, 94, 95, 96, 97):               # trimmed lengths on 31-base block edges and 32-base word edges
        row(rand_seq(rng, tot + 2 * cut))
        row(rand_seq(rng, tot), klen=30)                           # (total lengths too; dropped where tot < 2 max_k)
    for l in (-5, 0, 5):                                           # left / right each of < 0, 0, > 0, both markers
        for r in (-5, 0, 5):
            row(rand_seq(rng, 2 * mk + 33), marker=1 + (l + r) % 2, left=l, right=r)
    row(rand_seq(rng, 2 * mk + 70), left=30000, right=-30000)
    row(rand_seq(rng, 2 * mk + 70), left=-30001, right=30001)        # (clamped by the attribute long)
    d = rand_seq(rng, 2 * mk + 90)                                 # a contig and its duplicate
    row(d, marker=1, left=-1, right=-1)
    row(d, marker=2, left=3, right=-1)
    e = rand_seq(rng, 31)                                          # two contigs sharing an end 31-mer
    row(e + rand_seq(rng, 2 * mk + 40))
    row(e + rand_seq(rng, 2 * mk + 55))
    row(rand_seq(rng, 2 * mk + 40) + e)
    # a 31-mer whose 30-base key equals a trimmed contig's key, in both sorted positions: u's end 31-mer at i = 0 is v's trimmed
    # start (the 31-mer records come first in the union, so it sorts ahead); and one that reaches the fold behind a long row
    # only through the reflected sort
    v = rand_seq(rng, 2 * mk + 80)
    row(v[cut:cut + 31] + rand_seq(rng, 2 * mk + 30))
    row(v)
    row(rand_seq(rng, 2 * mk + 30) + v[len(v) - cut - 31:len(v) - cut])
    core = rand_seq(rng, 30)                                       # one-base rows of one key with all four bases (the end 31-mers)
    for ch in "TGCA":
        row(core + ch + rand_seq(rng, 2 * mk + 20))
    for ch in "GATC":
        row(rand_seq(rng, 2 * mk + 20) + ch + core)
    row(rand_seq(rng, 2 * mk + 50), tuple_text=True)
    s = rand_seq(rng, 2 * mk + 50)
    row(s[:40] + "N" + s[41:100] + "n" + s[101:])                  # letters that are not ACGT read as T
    if big:
        row(rand_seq(rng, 3000 + int(rng.integers(0, 64))), marker=1, klen=mk - 1)
        row(rand_seq(rng, 3100 + int(rng.integers(0, 64))), marker=2, klen=31)
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


def compare(ref, mod, what):
    if ref != mod:
        i = next((j for j, (x, y) in enumerate(zip(ref, mod)) if x != y), min(len(ref), len(mod)))
        raise AssertionError(f"{what}: the string model differs from the reference at row {i} of {len(ref)} / {len(mod)}: "
                             f"{ref[i:i + 2]} vs {mod[i:i + 2]}")


def run_case(name, p, P, rows, hits, rng):
    st, ps, perms, kmers, order, passes, text = ref_pipeline(rows, p, P)
    st2, ps2, _, kmers2, _, passes2, text2 = ref_pipeline(rows, p, P, shuffle=rng)
    assert kmers2 == kmers and sorted(st2["union"]) == sorted(st["union"]) and st2["union"] != st["union"], name + ": the shuffled run"
    for s in ("fold1", "reflected", "sort2", "fold2"):             # the proof that the order contract does not need groupBy's order
        assert st2[s] == st[s] and ps2.get(s) == ps.get(s), f"{name}: stage {s} depends on the order of the distinct 31-mers"
    assert passes2 == passes and text2 == text, name + ": the loop depends on the order of the distinct 31-mers"
    mst, mps, mk, mpasses = fm.run_stages(rows, p, P, hits)
    compare(kmers, mk, name + " 31-mers")
    for s in fm.STAGES:
        compare(st[s], mst[s], f"{name} {s}")
        if s in ps:
            compare(ps[s], mps[s], f"{name} {s} partition starts")
    assert len(passes) == len(mpasses) == 1 + fm.loop_rounds(p)
    for i, (a, b) in enumerate(zip(passes, mpasses)):              # step 9 IS the dynamic-k pass: every loop stage agrees
        compare(a, b, f"{name} loop pass {i}")
    assert text == fm.to_text(mpasses[-1]), name + " text"
    for q in range(P):                                             # the closed form of both folds
        for a, b in (("sort1", "fold1"), ("sort2", "fold2")):
            assert fm.fold_closed_form(st[a][ps[a][q]:ps[a][q + 1]]) == st[b][ps[b][q]:ps[b][q + 1]], f"{name}: closed form of {b}"
    assert fm.kmer_set(kmers, st["long"], "sorted")[:len(order)] == sorted(st["union"][:len(order)])
    merging = sum(1 for a, b in zip([st["fold2"]] + passes, passes) if len(b) < len(a))
    return (st, ps, perms, kmers, order, passes, text), merging


def store(out, name, p, P, rows, res):
    st, ps, perms, kmers, order, passes, text = res
    out[name + "/meta"] = np.array([p["max_k"], p["scramble"], p["max_iteration"], P, len(passes)], np.int64)
    out[name + "/rows"], out[name + "/rows_off"] = pack_strings([r + "\n" for r in rows])
    out[name + "/kmers"], out[name + "/kmers_off"] = pack_strings(kmers)

    def records(tag, recs):
        out[f"{name}/{tag}_key"], out[f"{name}/{tag}_key_off"] = pack_strings([r[0] for r in recs])
        out[f"{name}/{tag}_ext"], out[f"{name}/{tag}_ext_off"] = pack_strings([r[2] for r in recs])
        out[f"{name}/{tag}_mlr"] = np.array([(r[1], r[3], r[4]) for r in recs], np.int32).reshape(-1, 3)

    kept, j = [], 0                                                # the binarizer keeps rows, in order
    for r in st["binarized"]:
        while fm.binarize([rows[j]], p) != [r]:
            j += 1
        kept.append(j)
        j += 1
    out[name + "/binarized_rows"] = np.array(kept, np.int32)
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
        else:
            records(s, recs)
        prev = recs
    for i, recs in enumerate(passes[:-1]):                         # (the last pass IS the text)
        records(f"pass{i}", recs)
    assert fm.from_text(text) == passes[-1]
    out[name + "/text"] = np.frombuffer(text.encode(), np.uint8)


def main():
    rng = np.random.default_rng(20261020)
    out, names, hits = {}, [], {}
    for name, mk, P, scramble, max_it, n_contigs, crafted, big in CASES:
        p = fm.default_params(mk, scramble=scramble, max_iteration=max_it)
        rows = make_rows(rng, mk, n_contigs, crafted, big)
        res, merging = run_case(name, p, P, rows, hits, rng)
        store(out, name, p, P, rows, res)
        names.append(name)
        st, passes = res[0], res[5]
        print(name, len(rows), "rows ->", {s: len(st[s]) for s in fm.STAGES}, "passes", [len(x) for x in passes], "merging passes", merging,
              "longest", max((len(r[0]) + len(r[2]) for r in passes[-1]), default=0), flush=True)
        if len(passes) >= 3 and merging < 3 and (crafted or P < 63):   # (63 partitions of a few rows hold one key each: every row
                                                                       # is a partition's first emission, all get one marker)
            raise SystemExit(f"{name}: the loop merges in {merging} passes only")
        if P == 63 and not crafted:                                # (few rows: empty partitions)
            assert any(a == b for a, b in zip(res[1]["sort1"], res[1]["sort1"][1:])), name + ": no empty partition"
    out["names"] = np.array(names)
    # (the left fold never sees a one-base row BEHIND a longer row of its key: the union puts the 31-mer records first and the
    # sort is stable; the right fold does, through the reflected sort)
    every = [f"{t} {b}" for t in "LR" for b in fm.FOLD_BRANCHES if (t, b) != ("L", "short_after_long_dropped")] + list(fm.LOOP_BRANCHES)
    print("branch hits", {b: hits.get(b, 0) for b in every}, flush=True)
    print("other labels", {b: h for b, h in hits.items() if b not in every}, flush=True)
    missing = [b for b in every if not hits.get(b)]
    if missing and "--allow-missing" not in sys.argv:
        raise SystemExit(f"branches never taken: {missing}")
    out["branch_names"] = np.array(every)
    out["branch_hits"] = np.array([hits.get(b, 0) for b in every], np.int64)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "fixing_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
