#!/usr/bin/env python3
"""Golden vectors for the mercy k-mer stage (Count_<k>_mercy) made by the REFERENCE'S OWN classes.

The seven operator classes of P/ReflexivDSDynamicMercyKmer.java that its driver (`assemblyFromKmer`, :157-322) runs are translated
mechanically (tools/java2py.py, from the reference's source text at generation time) and driven in the driver's order:
ReverseComplementKmerBinaryExtractionFromDataset and DynamicKmerBinarizer -> union -> sort("seed") -> RamenReadExtraction -> sort("ID")
-> RamenReadRangeCal; FastqTuple2Dataset -> union -> sort("ID") -> ExtractMercyKmerFromRead -> DSBinaryKmerToString.  What sits between
two classes is Spark's; here: ONE logical partition (equal seeds and equal IDs never straddle a range partition), every sort stable,
array<long> ordered element by element as SIGNED longs, and BOTH orders of each union -- the generator asserts that the two agree.  No
reference code is stored.

Output: tests/golden/mercy_vectors.npz -- per case the Count_<k> rows, the reads, [k, front_clip, end_clip], the hit list per read
(RamenReadExtraction's rows behind sort("ID"), the index column), the kept ranges per read (RamenReadRangeCal's markers as pairs
left, right = a + 1, b), the final text and [reads, hits, ranges, rows]; `refused_k`: the k of 8..31 at which the classes throw or
disagree with themselves across the union orders (rows [k, what]; empty when there is none)."""
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
from make_dedup_vectors import blocks_of, rc, rand_seq, sgn  # noqa: E402
from make_ksort_vectors import pack_strings  # noqa: E402

REF = os.environ.get("RFX_REFERENCE", "/root/reference") + "/src/main/java/uni/bielefeld/cmg/reflexiv/pipeline/"
CLASSES = ["ReverseComplementKmerBinaryExtractionFromDataset", "DynamicKmerBinarizer", "RamenReadExtraction", "RamenReadRangeCal",
           "FastqTuple2Dataset", "ExtractMercyKmerFromRead", "DSBinaryKmerToString"]
_cls = {}
EXTRA = {}                 # what a case stores beside its stages (the planted genome and its stretches)


def op(name, param):
    if not _cls:
        _cls.update(jp.translate_classes(REF + "ReflexivDSDynamicMercyKmer.java", CLASSES))
    return _cls[name](jp.Outer(param, _cls))


def ref_param(k, front_clip, end_clip):
    param = make_param(k, frontClip=front_clip, endClip=end_clip)
    param.setKmerListArray(str(k))
    param.setKmerListHash(str(k))
    return param


def marker3(a):
    """a range marker as RamenReadRangeCal.getLeftMarker / getRightMarker read it back"""
    a = u64(a)
    left = (a >> 32) & 0x3FFFFFFF
    right = sgn((a & 0xFFFFFFFF) << 32) >> 32
    return 30000 - left if left > 30000 else left, 30000 - right if right > 30000 else right


def mercy_pipeline(count_rows, reads, k, front_clip, end_clip, solid_first=True):
    """count_rows: 'KMER,count' strings, reads: strings -> (hits per read, ranges per read, text)"""
    param = ref_param(k, front_clip, end_clip)
    n = len(reads)
    tuples = [jp.JTuple(r, jp._L(i)) for i, r in enumerate(reads)]                         # zipWithIndex
    seeds = drain(op("ReverseComplementKmerBinaryExtractionFromDataset", param).call(jp.JIter(tuples)))      # (seed, ID, index)
    rows0 = [jp.Row(r.split(",", 1)) for r in count_rows]                                   # spark.read().csv: two string columns
    solid = drain(op("DynamicKmerBinarizer", param).call(jp.JIter(rows0)))                  # (seed, ID, -1)
    cur = solid + seeds if solid_first else seeds + solid
    cur = sorted(cur, key=lambda r: tuple(sgn(w) for w in blocks_of(r.getSeq(0))))          # sort("seed"): signed, stable
    cur = drain(op("RamenReadExtraction", param).call(jp.JIter(cur)))                       # (ID, index)
    cur = sorted(cur, key=lambda r: r.getLong(0).v)                                         # sort("ID")
    hit_rows = [(int(r.getLong(0).v), int(r.getLong(1).v)) for r in cur]
    ranges = drain(op("RamenReadRangeCal", param).call(jp.JIter(cur))) if cur else []      # (ID, markers); it throws on an empty partition
    blocks = drain(op("FastqTuple2Dataset", param).call(jp.JIter(tuples)))                  # (ID, blocks)
    cur = blocks + ranges if solid_first else ranges + blocks
    cur = sorted(cur, key=lambda r: r.getLong(0).v)                                         # sort("ID")
    cur = drain(op("ExtractMercyKmerFromRead", param).call(jp.JIter(cur)))                  # (kmer blocks, count)
    out = drain(op("DSBinaryKmerToString", param).call(jp.JIter(cur)))
    return hit_rows, ranges, "".join(f"{r.vals[0]},{jp._tostr(r.vals[1])}\n" for r in out), n


def decode(hit_rows, ranges, n):
    """-> (hits per read, ascending; kept ranges per read as (left, right) = (a + 1, b))"""
    hits = [[] for _ in range(n)]
    for i, p in hit_rows:
        hits[i].append(p)
    kept = [[] for _ in range(n)]
    for r in ranges:
        m = r.get(1)
        m = [w.v for w in (m.items if isinstance(m, jp.Seq) else m)]
        kept[abs(int(r.getLong(0).v))] += [marker3(x) for x in m[2:]]
    return [sorted(h) for h in hits], kept


def run_both(rows, reads, k, fc, ec):
    """both union orders; they must agree"""
    a = mercy_pipeline(rows, reads, k, fc, ec, True)
    b = mercy_pipeline(rows, reads, k, fc, ec, False)
    da, db = decode(*a[:2], len(reads)), decode(*b[:2], len(reads))
    assert da == db and a[2] == b[2], "the two union orders disagree"
    return da[0], da[1], a[2]


def canon(s):
    s = "".join(c if c in "ACG" else "T" for c in s)
    return min(s, rc(s))


def solid_rows(rng, reads_and_hits, k, extra=()):
    """the count rows that make exactly the chosen windows solid (random collisions aside), as the counter writes them, shuffled"""
    ks = sorted({canon(r[p:p + k]) for r, hs in reads_and_hits for p in hs if 0 <= p <= len(r) - k})
    rows = [f"{s},{int(rng.integers(2, 41))}" for s in ks] + list(extra)
    return [rows[i] for i in rng.permutation(len(rows))]


def crafted(rng, k, fc, ec):
    """-> (reads with the windows chosen to be solid, the names of what must give rows)"""
    rh = []
    for g in range(1, k + 4):                                      # every gap size 1 .. k + 3, two of them in one read for some
        r = rand_seq(rng, fc + 2 + g + 1 + k + 3 + ec)
        rh.append((r, [fc + 2, fc + 2 + g + 1]))
    for n in (150, 151, 64, 65, 63):                               # a gap at the first and at the last possible window
        r = rand_seq(rng, n)
        last = n - ec - k
        if last - fc > 12:
            rh.append((r, [fc, fc + 3, last - 5, last]))
    for n in (k - 1, k, k + 1, k + 2, 16, 17, 18, 31, 32, 33, 63, 64, 65, 150, 151):      # the read lengths: first and last window solid
        r = rand_seq(rng, n)
        rh.append((r, [fc, n - ec - k]))
    r = rand_seq(rng, 100)
    rh.append((r, []))                                             # no window solid
    r = rand_seq(rng, 100)
    rh.append((r, [40]))                                           # one
    r = rand_seq(rng, 100)
    rh.append((r, list(range(0, 100 - k + 1))))                    # all
    r = rand_seq(rng, 120)
    rh.append((r, [fc + 1, fc + 6, fc + 7, fc + 40, fc + 41 + k, fc + 80]))       # several gaps, one of them of k bases (skipped)
    both = [(rc(r), [len(r) - k - p for p in hs]) for r, hs in rh[::3]]             # the other strand
    rh += both
    r = rand_seq(rng, 90)
    rh.append((r[:fc + 10] + "N" + r[fc + 11:fc + 14] + "n" + r[fc + 15:], [fc + 2, fc + 30]))      # N and lower case inside a gap
    r = rand_seq(rng, 90)
    rh.append((r[:30] + r[30:60].lower() + r[60:], [fc + 1, 90 - ec - k]))         # lower case reads as T
    for n, a in ((31, 31), (32, 31), (40, 31), (40, 30), (80, 31), (80, 30)):      # leading A: 31 of them and 32 bases or more give nothing
        r = "A" * a + ("C" if a < n else "") + rand_seq(rng, max(0, n - a - 1))
        rh.append((r[:n], [fc, n - ec - k]))
    return rh


def planted(rng, k=31, L=2000, read_len=100):
    """a genome, reads at coverage >= 2 everywhere except two stretches that exactly one read crosses -> (genome, reads, stretches)"""
    g = rand_seq(rng, L)
    stretches = [(700, 720), (1400, 1433)]
    starts = []
    for lo, hi in ((0, 700), (720, 1400), (1433, L)):
        tiles = list(range(lo, hi - read_len + 1, 10))
        if tiles[-1] != hi - read_len:
            tiles.append(hi - read_len)
        starts += [tiles[0]] + tiles + [tiles[-1]]                 # the tiles at an edge twice: every window of theirs is seen twice
    starts += [s - 35 for s, _ in stretches]                       # the one read across each stretch
    reads = [g[s:s + read_len] for s in starts]
    reads = [rc(r) if i % 3 == 1 else r for i, r in enumerate(reads)]
    return g, [reads[i] for i in rng.permutation(len(reads))], stretches


def counted_twice(reads, k):
    seen = {}
    for r in reads:
        for p in range(len(r) - k + 1):
            c = canon(r[p:p + k])
            seen[c] = seen.get(c, 0) + 1
    return sorted(s for s, c in seen.items() if c >= 2)


def case_list(rng):
    """(name, rows, reads, k, fc, ec, must give rows)"""
    cases = []
    for k in (8, 15, 16, 21, 23, 30, 31):
        for fc, ec in ((0, 0), (1, 2)) if k in (15, 31) else ((0, 0),):
            rh = crafted(rng, k, fc, ec)
            none = next(r for r, hs in rh if hs == [] and len(r) == 100)
            s = canon(none[10:10 + k])                             # a window of the read without hits, in its NON-canonical form: no hit
            extra = [f"{rand_seq(rng, k + 3)},9", f"{rand_seq(rng, k - 1)},4", f"{rc(s)},5"]       # rows of another length are dropped
            wrapped = canon(rh[0][0][fc + 2:fc + 2 + k])           # one solid row as tuple text: "(KMER,7)"
            rows = [f"({wrapped},7)" if r.split(",")[0] == wrapped else r for r in solid_rows(rng, rh, k, extra)]
            cases.append((f"k{k}_c{fc}_{ec}", rows, [r for r, _ in rh], k, fc, ec, True))
    rh = crafted(rng, 21, 0, 0)
    rows = solid_rows(rng, rh, 21)
    reads = [r for r, _ in rh]
    cases.append(("k21_front_clip_above_length", rows, reads, 21, 200, 0, False))
    cases.append(("k21_clips_leave_no_window", rows, reads, 21, 0, 140, False))
    cases.append(("k21_clips_40_0", rows, reads, 21, 40, 0, True))
    cases.append(("k21_clips_0_40", rows, reads, 21, 0, 40, True))
    g, reads, stretches = planted(rng)
    EXTRA["planted_k31/genome"] = np.frombuffer(g.encode(), np.uint8)
    EXTRA["planted_k31/stretches"] = np.array(stretches, np.int64)
    cases.append(("planted_k31", [f"{s},2" for s in counted_twice(reads, 31)], reads, 31, 0, 0, True))
    return cases


def sweep(rng):
    """every k of 8..31 on a small random input: the k at which the classes throw or the union orders disagree"""
    cases, refused = [], []
    for k in range(8, 32):
        rh = crafted(rng, k, 0, 0)[::4]
        rows, reads = solid_rows(rng, rh, k), [r for r, _ in rh]
        try:
            run_both(rows, reads, k, 0, 0)
            cases.append((f"sweep_k{k}", rows, reads, k, 0, 0, True))
        except Exception as e:                                     # the classes threw, or disagree with themselves
            refused.append((k, 0 if isinstance(e, AssertionError) else 1))
    return cases, np.array(refused, np.int64).reshape(-1, 2)


def run_case(c):
    name, rows, reads, k, fc, ec, must = c
    hits, kept, text = run_both(rows, reads, k, fc, ec)
    return name, hits, kept, text


def main():
    rng = np.random.default_rng(20261020)
    cases = case_list(rng)
    more, refused = sweep(rng)
    cases += more
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 1
    if jobs > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(jobs) as pool:
            results = pool.map(run_case, cases, chunksize=1)
    else:
        results = [run_case(c) for c in cases]
    out = {"names": np.array([c[0] for c in cases]), "refused_k": refused}
    out.update(EXTRA)
    for (name, rows, reads, k, fc, ec, must), (_, hits, kept, text) in zip(cases, results):
        n_rows = text.count("\n")
        assert not must or n_rows > 0, (name, "gives no rows")
        out[name + "/params"] = np.array([k, fc, ec], np.int64)
        out[name + "/rows"], out[name + "/rows_off"] = pack_strings([r + "\n" for r in rows])
        out[name + "/reads"], out[name + "/reads_off"] = pack_strings(reads)
        out[name + "/hits"] = np.array([p for h in hits for p in h], np.int32)
        out[name + "/hits_off"] = np.cumsum([0] + [len(h) for h in hits]).astype(np.int64)
        out[name + "/ranges"] = np.array([x for kr in kept for x in kr], np.int32).reshape(-1, 2)
        out[name + "/ranges_off"] = np.cumsum([0] + [len(kr) for kr in kept]).astype(np.int64)
        out[name + "/text"] = np.frombuffer(text.encode(), np.uint8)
        out[name + "/totals"] = np.array([len(reads), sum(len(h) for h in hits), sum(len(kr) for kr in kept), n_rows], np.int64)
        print(name, len(rows), "count rows,", out[name + "/totals"].tolist(), flush=True)
    print("refused_k", refused.tolist(), flush=True)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "mercy_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
