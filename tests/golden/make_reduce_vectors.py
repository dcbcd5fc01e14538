#!/usr/bin/env python3
"""Golden vectors for the k-mer reduction stage (Count_<k>_reduced) made by the REFERENCE'S OWN classes.

The operator classes of P/ReflexivDSDynamicKmerRuduction.java that its driver (`assemblyFromKmer`, :143-287) runs are
translated mechanically (tools/java2py.py, from the reference's source text at generation time) and driven in the driver's
order: DynamicKmerBinarizerFromSorted on both inputs -> union (the longer set first) ->
LeftLongerToShorterComparisonPreparation -> sort("k-1") -> LeftLongerKmerVariantAdjustment ->
RightLongerToShorterComparisonAndNeutralizationPreparation -> sort("k-1") ->
RightLongerKmerVariantAdjustmentAndNeutralization -> DSSubKmerToFullKmer -> sort("k") -> ShorterKmerNeutralization ->
DSBinaryFullKmerArrayToStringShort / ...Long.  What sits between two classes is Spark's; here: every sort stable, array<long>
ordered element by element as SIGNED longs (a prefix first), P logical partitions cut at floor(p*n/P) moved forward past
equal keys (make_reference_vectors.partition_starts), a fresh operator instance per partition.  No reference code is stored.

Every stage of every case is ALSO computed by the string model (tests/reduce_model.py) and must agree; the model counts the
branches the two adjustments take and the generator fails if a branch is never taken.

Output: tests/golden/reduce_vectors.npz -- per case the two inputs' rows, the record set behind every stage (a sort as
the permutation of the stage before it, an adjustment's / the neutralizer's output as indices into its input + extension +
attributes), the partition starts in and out of the partitioned operators, and both texts; a case that runs another
case's rows under another max_k only names it (max_k decides the NAME of the second output, nothing else).
`probe_k`: what the classes do where k or k - 1 is a multiple of 31, rows [k1, k2, 1 if every stage agrees with the string
model / 0 if a stage differs / -1 if a class threw]."""
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
import reduce_model as rm  # noqa: E402
from make_reference_vectors import make_param, drain, u64, partition_starts  # noqa: E402
from make_dedup_vectors import blocks_of, blocks_to_seq, rand_seq  # noqa: E402
from make_dynamic_vectors import as_seq_rows, key_of  # noqa: E402
from make_ksort_vectors import attr3, pack_strings  # noqa: E402

REF = os.environ.get("RFX_REFERENCE", "/root/reference") + "/src/main/java/uni/bielefeld/cmg/reflexiv/pipeline/"
CLASSES = ["DynamicKmerBinarizerFromSorted", "LeftLongerToShorterComparisonPreparation", "LeftLongerKmerVariantAdjustment",
           "RightLongerToShorterComparisonAndNeutralizationPreparation", "RightLongerKmerVariantAdjustmentAndNeutralization",
           "DSSubKmerToFullKmer", "ShorterKmerNeutralization", "DSBinaryFullKmerArrayToStringShort",
           "DSBinaryFullKmerArrayToStringLong"]
PAIRS = ((8, 9), (23, 31), (30, 31), (31, 41), (33, 34), (53, 67), (64, 65), (95, 97), (97, 124))
PROBE = ((31, 41), (23, 31), (32, 41), (23, 32), (62, 70), (41, 62), (63, 70), (41, 63), (93, 100), (70, 93), (94, 100), (70, 94))
_cls = {}


def op(name, param):
    if not _cls:
        _cls.update(jp.translate_classes(REF + "ReflexivDSDynamicKmerRuduction.java", CLASSES))
    return _cls[name](jp.Outer(param, _cls))


def ref_param(k1, k2, max_k):
    klist = sorted({k1, k2, max_k})
    param = make_param(k1)
    param.kmerSize1, param.kmerSize2 = jp._I(k1), jp._I(k2)
    kl = ",".join(str(x) for x in klist)
    param.setKmerListArray(kl)
    param.setKmerListHash(kl)
    return param


def rec3(row):
    m, l, r = attr3(row.vals[1].v)
    return blocks_to_seq(blocks_of(row.vals[0])), blocks_to_seq((u64(row.vals[2].v),)), m, l, r


def rec2(row):
    return (blocks_to_seq(blocks_of(row.vals[0])), "") + attr3(row.vals[1].v)


def text_rows(rows):
    return [jp.Row(r.rstrip("\n").split(",", 1)) for r in rows]


def ref_pipeline(rows_short, rows_long, k1, k2, max_k, P):
    """-> ({stage: records}, {stage: partition starts}, {sort stage: permutation}, text of k1, text of k2)"""
    param = ref_param(k1, k2, max_k)
    st, ps, perms = {}, {}, {}
    one = lambda name, rows: drain(op(name, param).call(jp.JIter(as_seq_rows2(rows))))       # noqa: E731

    def parts(name, rows, tag_in, tag_out):
        cuts = partition_starts([key_of(r) for r in rows], P)
        out, ost = [], [0]
        for p in range(P):
            out += drain(op(name, param).call(jp.JIter(as_seq_rows2(rows[cuts[p]:cuts[p + 1]]))))
            ost.append(len(out))
        ps[tag_in], ps[tag_out] = cuts, ost
        return out

    def sort(rows, name):
        perm = sorted(range(len(rows)), key=lambda i: key_of(rows[i]))                      # stable; signed; a prefix first
        perms[name] = perm
        return [rows[i] for i in perm]

    cur = drain(op("DynamicKmerBinarizerFromSorted", param).call(jp.JIter(text_rows(rows_long))))
    cur += drain(op("DynamicKmerBinarizerFromSorted", param).call(jp.JIter(text_rows(rows_short))))
    st["union"] = [rec2(r) for r in cur]
    cur = one("LeftLongerToShorterComparisonPreparation", cur)
    st["left_prep"] = [rec3(r) for r in cur]
    cur = sort(cur, "left_sort")
    st["left_sort"] = [rec3(r) for r in cur]
    cur = parts("LeftLongerKmerVariantAdjustment", cur, "left_sort", "left_adj")
    st["left_adj"] = [rec3(r) for r in cur]
    cur = one("RightLongerToShorterComparisonAndNeutralizationPreparation", cur)
    st["right_prep"] = [rec3(r) for r in cur]
    cur = sort(cur, "right_sort")
    st["right_sort"] = [rec3(r) for r in cur]
    cur = parts("RightLongerKmerVariantAdjustmentAndNeutralization", cur, "right_sort", "right_adj")
    st["right_adj"] = [rec3(r) for r in cur]
    cur = one("DSSubKmerToFullKmer", cur)
    st["full"] = [rec2(r) for r in cur]
    cur = sort(cur, "full_sort")
    st["full_sort"] = [rec2(r) for r in cur]
    cur = parts("ShorterKmerNeutralization", cur, "full_sort", "neutral")
    st["neutral"] = [rec2(r) for r in cur]
    t1 = drain(op("DSBinaryFullKmerArrayToStringShort", param).call(jp.JIter(as_seq_rows2(cur))))
    t2 = drain(op("DSBinaryFullKmerArrayToStringLong", param).call(jp.JIter(as_seq_rows2(cur))))
    return st, ps, perms, "".join(f"{r.vals[0]},{r.vals[1]}\n" for r in t1), "".join(f"{r.vals[0]},{r.vals[1]}\n" for r in t2)


def as_seq_rows2(rows):
    """rows as the next Spark stage reads them: the array column comes back as Seq (two- and three-column rows)"""
    out = []
    for r in rows:
        v = list(r.vals)
        if isinstance(v[0], list):
            v[0] = jp.Seq(v[0])
        out.append(jp.Row(v))
    return out


MARK = (-1, -1, -3, 1, 2, 7, 100, 30000)


def make_rows(rng, k1, k2, big):
    """the two Count_<k>_sorted files of a small genome + the crafted rows of the issue"""
    short, long_, seen = [], [], set()

    def attr():
        return f"1|{int(rng.choice(MARK))}|{int(rng.choice(MARK))}"

    def add(kmer, dst, a=None):
        if kmer in seen:
            return
        seen.add(kmer)
        dst.append(f"{kmer},{a or attr()}")

    g = rand_seq(rng, (150 if big else 60) + k2)
    n = len(g)
    for i in range(0, n - k1 + 1):                                 # the short k-mers of the first two thirds
        if i < 2 * n // 3:
            add(g[i:i + k1], short)
    for i in range(n // 3, n - k2 + 1):                            # the long ones of the last two thirds
        add(g[i:i + k2], long_)
    d = k2 - k1
    for rep in range(36 if big else 14):
        core = rand_seq(rng, k1)                                   # a short row with 0..3 longer rows on its left / right
        nl, nr = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        if rep % 4 != 3:
            add(core, short)                                       # (rep % 4 == 3: longer rows without their short row)
        for j in range(nl):                                        # left: X + core[:-1] + e, e equal or not
            e = core[-1] if rng.random() < 0.5 else "ACGT"[int(rng.integers(0, 4))]
            add(rand_seq(rng, d) + core[:-1] + e, long_)
        for j in range(nr):                                        # right: f + core[1:] + Y, f equal or not
            f = core[0] if rng.random() < 0.5 else "ACGT"[int(rng.integers(0, 4))]
            add(f + core[1:] + rand_seq(rng, d), long_)
    for rep in range(10 if big else 4):                            # two short rows that share a longer row on the right / left
        core = rand_seq(rng, k1 - 1)
        tail = rand_seq(rng, d)
        for f in rng.permutation(4)[:int(rng.integers(1, 4))]:
            add("ACGT"[f] + core, short)
        for f in rng.permutation(4)[:int(rng.integers(1, 4))]:
            add("ACGT"[f] + core + tail, long_)
        core = rand_seq(rng, k1 - 1)
        head = rand_seq(rng, d)
        for e in rng.permutation(4)[:int(rng.integers(1, 4))]:
            add(core + "ACGT"[e], short)
        for e in rng.permutation(4)[:int(rng.integers(1, 4))]:
            add(head + core + "ACGT"[e], long_)
    s = rand_seq(rng, k2)                                          # the neutralizer's drop stretch: a short row 40 times
    long_.append(f"{s},{attr()}")
    dup = [f"{s[:k1]},{attr()}" for _ in range(40)]
    for j, q in enumerate(sorted(rng.integers(0, len(short) + 1, 40))):
        short.insert(int(q) + j, dup[j])
    short.append(f"({rand_seq(rng, k1)},1|-5|6)")                  # tuple text
    long_.append(f"({rand_seq(rng, k2)},1|30001|-30001)")           # clamped attributes
    short.append(f"{rand_seq(rng, k1 + 1 if k1 + 1 != k2 else k1 - 1)},1|2|3")                # an unlisted length: dropped
    long_.append(f"{rand_seq(rng, k2 + 2)},1|2|3")
    s = rand_seq(rng, k1)
    short.append(f"{s[:2]}N{s[3:]},1|4|4")                         # a letter that is not ACGT reads as T
    return short, long_


def compare(ref, mod, what):
    if ref != mod:
        i = next((j for j, (x, y) in enumerate(zip(ref, mod)) if x != y), min(len(ref), len(mod)))
        raise AssertionError(f"{what}: the string model differs from the reference at row {i} of {len(ref)} / {len(mod)}: "
                             f"{ref[i:i + 2]} vs {mod[i:i + 2]}")


def run_case(name, k1, k2, max_k, P, rows_s, rows_l, hits):
    st, ps, perms, t1, t2 = ref_pipeline(rows_s, rows_l, k1, k2, max_k, P)
    mst, mps = rm.run_stages(rows_s, rows_l, k1, k2, P, hits)
    for s in rm.STAGES:
        compare(st[s], mst[s], f"{name} {s}")
        if s in ps:
            compare(ps[s], mps[s], f"{name} {s} partition starts")
    m1, m2 = rm.to_text(mst["neutral"], k1), rm.to_text(mst["neutral"], k2)
    assert (t1, t2) == (m1, m2), name + " texts"
    return st, ps, perms, t1, t2


def store(out, name, k1, k2, max_k, P, rows_s, rows_l, res):
    st, ps, perms, t1, t2 = res
    out[name + "/meta"] = np.array([k1, k2, max_k, P], np.int64)
    out[name + "/rows_short"], out[name + "/rows_short_off"] = pack_strings(rows_s)
    out[name + "/rows_long"], out[name + "/rows_long_off"] = pack_strings(rows_l)
    prev = None
    for s in rm.STAGES:
        recs = st[s]
        out[f"{name}/{s}_mlr"] = np.array([r[2:] for r in recs], np.int32).reshape(-1, 3)
        if s in ps:
            out[f"{name}/{s}_ps"] = np.array(ps[s], np.int64)
        if s in perms:
            out[f"{name}/{s}_perm"] = np.array(perms[s], np.int32)
        elif s in ("left_adj", "right_adj", "neutral"):           # every output row is an input row, in order, maybe edited
            src, j = [], 0
            for r in recs:
                while prev[j][0] != r[0] or (s == "neutral" and prev[j] != r):
                    j += 1
                src.append(j)
                j += 1
            out[f"{name}/{s}_from"] = np.array(src, np.int32)
            out[f"{name}/{s}_ext"] = np.frombuffer("".join(r[1] for r in recs).encode(), np.uint8)
        else:
            out[f"{name}/{s}_key"], out[f"{name}/{s}_key_off"] = pack_strings([r[0] for r in recs])
            out[f"{name}/{s}_ext"] = np.frombuffer("".join(r[1] for r in recs).encode(), np.uint8)
        prev = recs
    out[name + "/text1"] = np.frombuffer(t1.encode(), np.uint8)
    out[name + "/text2"] = np.frombuffer(t2.encode(), np.uint8)


def probe(rng):
    res = []
    for k1, k2 in PROBE:
        rows_s, rows_l = make_rows(rng, k1, k2, False)
        try:
            run_case(f"probe{k1}_{k2}", k1, k2, k2, 2, rows_s, rows_l, None)
            res.append((k1, k2, 1))
        except AssertionError:
            res.append((k1, k2, 0))
        except Exception:                                          # a class threw
            res.append((k1, k2, -1))
    return np.array(res, np.int64)


def main():
    rng = np.random.default_rng(20261019)
    out, names, hits = {}, [], {}
    plist = (1, 2, 7, 63)
    for ci, (k1, k2) in enumerate(PAIRS):
        rows_s, rows_l = make_rows(rng, k1, k2, k2 <= 41)
        for P in (plist if (k1, k2) == (23, 31) else (plist[ci % 4],)):
            name = f"k{k1}_{k2}_P{P}"
            res = run_case(name, k1, k2, k2, P, rows_s, rows_l, hits)
            store(out, name, k1, k2, k2, P, rows_s, rows_l, res)
            names.append(name)
            print(name, len(rows_s), "+", len(rows_l), "rows ->", {s: len(res[0][s]) for s in ("union", "left_adj", "right_adj", "neutral")},
                  len(res[3]), "+", len(res[4]), "bytes", flush=True)
            if P == plist[ci % 4]:                                 # the twin: a longer k list; it changes the second output's name only
                twin = f"{name}_m{k2 + 10}"
                res2 = run_case(twin, k1, k2, k2 + 10, P, rows_s, rows_l, None)
                assert res2 == res, twin
                out[twin + "/meta"] = np.array([k1, k2, k2 + 10, P], np.int64)
                out[twin + "/seqs_from"] = np.array(name)
                names.append(twin)
    out["names"] = np.array(names)
    every = [t + b for t in "LR" for b in ("SSS", "SSL_shift", "SSL_two", "SLS_edit", "SLS_shift", "SLS_two", "SLL_three", "SLL_edit",
                                           "SLL_shift", "LSS_edit", "LSS_two", "LSL_three", "LSL_edit", "LSL_shift", "LSL_two", "LLS_three",
                                           "LLS_shift", "LLS_two", "LLL", "F_SL_edit", "F_LS_edit", "F_LS_none", "F_SS", "F_LL", "F_SL", "F_one")]
    every += ["RSLL_three_drop", "RLSL_three_drop", "RLLS_three_drop"]
    print("branch hits", {b: hits.get(b, 0) for b in every}, flush=True)
    missing = [b for b in every if not hits.get(b)]
    if missing and "--allow-missing" not in sys.argv:
        raise SystemExit(f"branches never taken: {missing}")
    out["branch_names"] = np.array(every)
    out["branch_hits"] = np.array([hits.get(b, 0) for b in every], np.int64)
    out["probe_k"] = probe(rng)
    print("probe_k", out["probe_k"].tolist(), flush=True)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "reduce_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
