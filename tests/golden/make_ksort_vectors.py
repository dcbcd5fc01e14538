#!/usr/bin/env python3
"""Golden vectors for the k-mer sorting stage (Count_<k>_sorted) made by the REFERENCE'S OWN classes.

The eight operator classes of P/ReflexivDSKmerLeftAndRightSorting.java that its driver (`assemblyFromKmer`, :105-243)
runs with param.bubble == true and param.minErrorCoverage > 0 are translated mechanically (tools/java2py.py, from the
reference's source text at generation time) and driven in the driver's order: DynamicKmerBinarizer -> filter(count <=
maxKmerCoverage) -> DSKmerReverseComplement -> DSForwardSubKmerExtraction -> sort("k-1") ->
DSFilterForkSubKmerWithErrorCorrection -> DSReflectedSubKmerExtractionFromForward -> sort("k-1") ->
DSFilterForkReflectedSubKmerWithErrorCorrection -> DSSubKmerToFullKmer -> DSBinaryFullKmerArrayToString.  What sits
between two classes is Spark's; here: ONE logical partition (both folds reset at a new key and equal keys never straddle
a range partition, so the result does not depend on the partition count), every sort stable, array<long> ordered element
by element as SIGNED longs.  No reference code is stored.

Output: tests/golden/ksort_vectors.npz -- per case the input rows, the record set behind each of steps 4, 5 (sort),
5 (fold), 6, 7 (sort), 7 (fold) and 8 as strings + attributes, and the final text (a sorted set is stored as the
permutation of the set before it; a case that runs another case's rows under another max_k stores its attributes and
names the case whose sequences it shares; the k-mers of step 8 are read from the text: tests/ksort_model.py `load_case` puts both back together); `refused_k`: what the classes do at
k = 32, 63, 94 ((k-1) % 31 == 0), rows [k, input rows, output rows, output rows that are no input k-mer or its RC] (at 63 and 94 the classes emit nothing)."""
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
from make_reference_vectors import make_param, drain, u64  # noqa: E402
from make_dedup_vectors import blocks_of, blocks_to_seq, rc, rand_seq  # noqa: E402

REF = os.environ.get("RFX_REFERENCE", "/root/reference") + "/src/main/java/uni/bielefeld/cmg/reflexiv/pipeline/"
CLASSES = ["DynamicKmerBinarizer", "DSKmerReverseComplement", "DSForwardSubKmerExtraction", "DSFilterForkSubKmerWithErrorCorrection",
           "DSReflectedSubKmerExtractionFromForward", "DSFilterForkReflectedSubKmerWithErrorCorrection", "DSSubKmerToFullKmer",
           "DSBinaryFullKmerArrayToString"]
STAGES = ("s4", "s5_sort", "s5_fold", "s6", "s7_sort", "s7_fold", "s8")
COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 16, 18, 29999, 30000, 30001)
_cls = {}


def op(name, param):
    if not _cls:
        _cls.update(jp.translate_classes(REF + "ReflexivDSKmerLeftAndRightSorting.java", CLASSES))
    return _cls[name](jp.Outer(param, _cls))


def sgn(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def attr3(a):
    """the attribute long as the reference reads it back (getReflexivMarker / getLeftMarker / getRightMarker)"""
    a = u64(a)
    left = (a >> 32) & 0x3FFFFFFF
    right = sgn((a & 0xFFFFFFFF) << 32) >> 32
    return a >> 62, 30000 - left if left > 30000 else left, 30000 - right if right > 30000 else right


def rec_of(row):
    """(k-1 blocks, attribute, extension long) -> (key, ext, marker, left, right)"""
    m, l, r = attr3(row.vals[1].v)
    return blocks_to_seq(blocks_of(row.vals[0])), blocks_to_seq((u64(row.vals[2].v),)), m, l, r


def ref_param(p, klist=None):
    klist = klist or ([p["k"]] if p["max_k"] == p["k"] else [p["k"], p["max_k"]])
    param = make_param(p["k"], minErrorCoverage=p["min_error_cov"], maxKmerCoverage=p["max_cov"])
    param.minRepeatFold = float(p["min_repeat_fold"])
    kl = ",".join(str(x) for x in klist)
    param.setKmerListArray(kl)
    param.setKmerListHash(kl)
    return param


def ksort_pipeline(rows, p, klist=None, stages=True):
    """rows: 'KMER,count' strings -> ({stage: records}, text); stages=False: the classes are run, their rows are not decoded"""
    param = ref_param(p, klist)
    dec = rec_of if stages else (lambda r: None)
    rows0 = [jp.Row(r.split(",", 1)) for r in rows]                                          # spark.read().csv: two string columns
    cur = drain(op("DynamicKmerBinarizer", param).call(jp.JIter(rows0)))                     # (long[] blocks, int count)
    cur = [r for r in cur if r.vals[1].v <= p["max_cov"]]                                    # filter(col("count").leq(maxKmerCoverage))
    cur = drain(op("DSKmerReverseComplement", param).call(jp.JIter(cur)))
    cur = drain(op("DSForwardSubKmerExtraction", param).call(jp.JIter(cur)))                 # (blocks, attribute, extension)
    st = {"s4": [dec(r) for r in cur]}
    order = lambda r: tuple(sgn(w) for w in blocks_of(r.vals[0]))                            # noqa: E731  sort("k-1"), signed, stable
    def sort(rows, name):                                                                   # the permutation is what is stored
        perm = sorted(range(len(rows)), key=lambda i: order(rows[i]))
        st[name + "_perm"] = perm
        return [rows[i] for i in perm]

    if p["bubble"]:
        cur = sort(cur, "s5_sort")
        st["s5_sort"] = [dec(r) for r in cur]
        cur = drain(op("DSFilterForkSubKmerWithErrorCorrection", param).call(jp.JIter(cur)))
        st["s5_fold"] = [dec(r) for r in cur]
        cur = drain(op("DSReflectedSubKmerExtractionFromForward", param).call(jp.JIter(cur)))
        st["s6"] = [dec(r) for r in cur]
        cur = sort(cur, "s7_sort")
        st["s7_sort"] = [dec(r) for r in cur]
        cur = drain(op("DSFilterForkReflectedSubKmerWithErrorCorrection", param).call(jp.JIter(cur)))
        st["s7_fold"] = [dec(r) for r in cur]
    cur = drain(op("DSSubKmerToFullKmer", param).call(jp.JIter(cur)))                        # (long[] k-mer blocks, attribute)
    st["s8"] = [(blocks_to_seq(blocks_of(r.vals[0])), "") + attr3(r.vals[1].v) for r in cur] if stages else None
    out = drain(op("DSBinaryFullKmerArrayToString", param).call(jp.JIter(cur)))
    return st, "".join(f"{r.vals[0]},{r.vals[1]}\n" for r in out)


def canon(s):
    return min(s, rc(s))


def make_rows(rng, k, long_run=False):
    """a counts file as the counter writes it (canonical k-mers, one row each) + the crafted rows of the issue"""
    g = rand_seq(rng, 300)
    seen, rows = set(), []

    def add(kmer, c, raw=False):
        if not raw:
            kmer = canon(kmer)
            if kmer in seen:
                return
            seen.add(kmer)
        rows.append(f"{kmer},{c}")

    for i in range(len(g) - k + 1):
        add(g[i:i + k], int(rng.integers(1, 41)))
    # forks: a (k-1)-mer with 1..4 successors and 0..3 predecessors, counts on both sides of E and F*x
    for ns in (1, 2, 3, 4):
        for npred in (0, 1, 2, 3):
            core = rand_seq(rng, k - 1)
            for b in rng.permutation(4)[:ns]:
                add(core + "ACGT"[b], int(rng.choice(COUNTS)))
            for b in rng.permutation(4)[:npred]:
                add("ACGT"[b] + core, int(rng.choice(COUNTS)))
    for a, b in ((4, 6), (5, 7), (5, 8), (8, 12), (9, 13), (1, 1), (1, 2), (7, 7), (30000, 30001), (29999, 30000)):
        core = rand_seq(rng, k - 1)
        x, y = rng.permutation(4)[:2]
        add(core + "ACGT"[x], a)
        add(core + "ACGT"[y], b)
        core = rand_seq(rng, k - 1)
        add("ACGT"[x] + core, b)
        add("ACGT"[y] + core, a)
    s = rand_seq(rng, k)
    rows.append(f"({s},7)")                                        # tuple text
    rows.append(f"{rand_seq(rng, k)},1234567890")                  # a 10-digit count
    s = rand_seq(rng, k)
    rows.append(f"{s[:3]}N{s[4:]},5")                              # a letter that is not ACGT
    rows.append(f"{rand_seq(rng, k).lower()},6")                   # lower case
    rows.append(f"{rand_seq(rng, k + 3)},9")                       # another length, in no case's k list: dropped
    if k % 2 == 0:
        h = rand_seq(rng, k // 2)
        rows.append(f"{h + rc(h)},10")                             # a palindrome: its own reverse complement
    s = rand_seq(rng, k)
    rows += [f"{s},12", f"{rc(s)},3"]                              # a k-mer listed together with its reverse complement
    if long_run:
        s = rand_seq(rng, k)
        run = [f"{s},{int(rng.choice(COUNTS + (20, 40)))}" for _ in range(600)]
        pos = sorted(rng.integers(0, len(rows) + 1, 600))
        for j, q in enumerate(pos):
            rows.insert(int(q) + j, run[j])
    return rows


def pack_strings(strs):
    off = np.zeros(len(strs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in strs])
    return np.frombuffer("".join(strs).encode(), np.uint8), off


def case_list():
    import ksort_model as km
    cases = []
    for k in (8, 23, 31, 33, 34, 62, 64, 65, 66, 95, 96, 97, 98, 124):
        for mk in ([k] if k == 97 else [k, 97]):                   # (max_k = k first: the other one shares its sequences)
            cases.append((f"k{k}_m{mk}", km.default_params(k, max_k=mk), False))
    cases.append(("k31_E4_F2", km.default_params(31, max_k=31, min_error_cov=4, min_repeat_fold=2.0), False))
    cases.append(("k31_maxcov12", km.default_params(31, max_k=95, max_cov=12), False))
    cases.append(("k33_bubble0", km.default_params(33, max_k=95, bubble=0), False))
    cases.append(("k41_longrun", km.default_params(41, max_k=95), True))
    return cases


def run_case(arg):
    name, p, rows = arg
    st, text = ksort_pipeline(rows, p)
    return name, p, rows, st, text


def refused(rng):
    out = []
    for k in (32, 63, 94):
        g = rand_seq(rng, 200 + k)
        kmers = sorted({canon(g[i:i + k]) for i in range(200)})
        rows = [f"{s},{int(rng.integers(1, 41))}" for s in kmers]
        both = set(kmers) | {rc(s) for s in kmers}
        p = dict(k=k, max_k=k, min_error_cov=8, max_cov=10000000, bubble=1, min_repeat_fold=1.5)
        try:
            st, text = ksort_pipeline(rows, p, stages=False)
            lines = text.splitlines()
            out.append((k, len(rows), len(lines), sum(1 for ln in lines if ln.split(",")[0] not in both)))
        except Exception:                                          # the classes threw
            out.append((k, len(rows), -1, -1))
    return np.array(out, np.int64)


def main():
    rng = np.random.default_rng(20261018)
    rows_of = {}                                                   # one row set per k (and one with the long run)
    cases = []
    for name, p, lr in case_list():
        if (p["k"], lr) not in rows_of:
            rows_of[(p["k"], lr)] = make_rows(rng, p["k"], lr)
        cases.append((name, p, rows_of[(p["k"], lr)]))
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 1
    if jobs > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(jobs) as pool:
            results = pool.map(run_case, cases, chunksize=1)
    else:
        results = [run_case(c) for c in cases]
    out = {"names": np.array([c[0] for c in cases])}
    done = {}
    for name, p, rows, st, text in results:
        out[name + "/params"] = np.array([p["k"], p["max_k"], p["min_error_cov"], p["max_cov"], p["bubble"]], np.int64)
        out[name + "/fold"] = np.array([p["min_repeat_fold"]], np.float64)
        base = f"k{p['k']}_m{p['k']}"                              # the same rows under another max_k: the sequences are stored once
        share = (name != base and base in done and st.keys() == done[base].keys() and
                 all([r[:2] for r in st[s]] == [r[:2] for r in done[base][s]] for s in STAGES if s in st))
        done[name] = st
        if share:
            out[name + "/seqs_from"] = np.array(base)
        else:
            out[name + "/rows"], out[name + "/rows_off"] = pack_strings([r + "\n" for r in rows])
        for s in STAGES:
            if s not in st:
                continue
            recs = st[s]
            out[f"{name}/{s}_mlr"] = np.array([r[2:] for r in recs], np.int32).reshape(-1, 3)
            if share:
                continue
            if s == "s8" and [r[0] for r in recs] == [ln.split(",")[0] for ln in text.splitlines()]:
                continue                                           # (the k-mers of step 8 are the text's)
            if s + "_perm" in st:                                  # a sort: the stage before it, permuted
                out[f"{name}/{s}_perm"] = np.array(st[s + "_perm"], np.int32)
                continue
            out[f"{name}/{s}_key"], out[f"{name}/{s}_key_off"] = pack_strings([r[0] for r in recs])
            out[f"{name}/{s}_ext"], out[f"{name}/{s}_ext_off"] = pack_strings([r[1] for r in recs])
        out[name + "/text"] = np.frombuffer(text.encode(), np.uint8)
        print(name, len(rows), "rows ->", {s: len(st[s]) for s in STAGES if s in st}, len(text), "bytes", flush=True)
    out["refused_k"] = refused(rng)
    print("refused_k", out["refused_k"].tolist(), flush=True)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "ksort_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
