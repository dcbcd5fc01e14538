"""String model of the reduction from reads (rfx_dev_reduce_reads / rfx_reduce_reads): the whole call, reads in and
the text of every Count_<k>_reduced out, composed of what is pinned elsewhere and of nothing else -- the CPU oracle's restatement of the
two counters (oracle/), tests/mercy_model.py, tests/ksort_model.py, tests/reduce_model.py -- and sharing no code with the library or
with the GPU tests.  Test infrastructure: imported by the tests and by tests/golden/make_reduce_reads_vectors.py only."""
import numpy as np

from oracle import oracle as O
from tests import ksort_model as K
from tests import mercy_model as M
from tests import reduce_model as R

DEFAULTS = dict(min_cov=2, max_cov=10000000, min_error_cov=8, min_repeat_fold=1.5, bubble=1, sensitive=0, front_clip=0, end_clip=0, P=8)


def e_rule(klist, min_cov, min_error_cov):
    """minErrorCoverage at the sorting of every k, from the orchestrator (Pipelines.java:1412-1416 before the first k's sorter, :1489-1493
    before every later k's): `if (k1 >= 61 && k2 < 81) E = 3 minKmerCoverage; else if (k1 >= 81) E = 3 minKmerCoverage` with k2 the
    SECOND k of the list, and for a later k `if (k >= 61 && k < 81) ... else if (k >= 81) ...`, which is k >= 61.  `param` is mutated, so
    a value once set stays for every k behind it."""
    out, E = [], min_error_cov
    for i, k in enumerate(klist):
        if i == 0:
            if k >= 61 and klist[1] < 81:
                E = 3 * min_cov
            elif k >= 81:
                E = 3 * min_cov
        elif 61 <= k < 81:
            E = 3 * min_cov
        elif k >= 81:
            E = 3 * min_cov
        out.append(E)
    return out


def key_letters(key, k):
    """one key of the counter as letters.  k <= 31: one word, two bits a base, the last base in the lowest bits.  k > 31: k // 32 + 1
    words; every word but the last holds 32 bases, the first in the highest bits; the last holds the k % 32 that remain, right-aligned"""
    words = [int(w) for w in np.atleast_1d(key)]
    out = []
    for j, w in enumerate(words):
        m = k - 32 * j if j == len(words) - 1 else 32
        for i in range(m):
            out.append("ACGT"[(w >> (2 * (m - 1 - i))) & 3])
    assert len(out) == k and len(words) == (1 if k <= 31 else k // 32 + 1)
    return "".join(out)


def _flat(reads):
    bases = np.frombuffer("".join(reads).encode(), np.uint8) if reads else np.zeros(0, np.uint8)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return bases, off


def counter_rows(reads, k, min_cov=2, max_cov=10000000, front_clip=0, end_clip=0):
    """Count_<k> as `KMER,count\\n` rows in the oracle's ascending key order (the skip rules of either counter are the oracle's)"""
    if not reads:
        return []
    bases, off = _flat(reads)
    if k <= 31:
        keys, counts, _ = O.count_filter(O.extract_canon(bases, off, k, front_clip, end_clip), min_cov, max_cov, O.TWIN_DS)
    else:
        keys, counts, _ = O.count_filter_w(O.extract_canon_w(bases, off, k, front_clip, end_clip), k, min_cov, max_cov)
    return [f"{key_letters(key, k)},{int(c)}\n" for key, c in zip(keys, counts)]


def sorter_rows(reads, k, prm):
    """what reaches the sorter of this k -> (rows, how many of them are mercy rows)"""
    rows = counter_rows(reads, k, prm["min_cov"], prm["max_cov"], prm["front_clip"], prm["end_clip"])
    extra = []
    if prm["sensitive"] and k <= 31 and reads:
        extra = M.mercy_text(rows, reads, k, prm["front_clip"], prm["end_clip"]).splitlines(keepends=True)
    return rows + extra, len(extra)


def model(reads, klist, Es=None, info=None, **params):
    """-> [the text of Count_<k>_reduced for every k, in list order].  Es: the E of every k instead of the rule's (to run a wrong rule on
    purpose).  info (a dict): filled with `rows` (the counter's row count per k), `mercy` (mercy rows per k) and `Es`."""
    prm = dict(DEFAULTS, **params)
    klist = [int(k) for k in klist]
    assert len(klist) >= 2 and all(a < b for a, b in zip(klist, klist[1:]))
    Es = list(Es) if Es is not None else e_rule(klist, prm["min_cov"], prm["min_error_cov"])
    assert len(Es) == len(klist)
    if info is not None:
        info.update(rows=[], mercy=[], Es=Es)
    if not reads:
        return ["" for _ in klist]
    out, prev = [], None
    for i, k in enumerate(klist):
        rows, n_mercy = sorter_rows(reads, k, prm)
        if info is not None:
            info["rows"].append(len(rows) - n_mercy)
            info["mercy"].append(n_mercy)
        cur = K.run_text(rows, K.default_params(k, max_k=klist[-1], min_error_cov=Es[i], max_cov=prm["max_cov"], bubble=prm["bubble"],
                                                min_repeat_fold=prm["min_repeat_fold"]))
        if i == 0:
            prev = cur
            continue
        short, prev = R.run_text(prev.splitlines(keepends=True), cur.splitlines(keepends=True), klist[i - 1], k, prm["P"])
        out.append(short)
    out.append(prev)
    return out


def first_capacity(n_reads, max_len, k, min_cov):
    """the rows the driver's first count has room for, restated from rr_sorted (reflexiv_amd/csrc/rfx_reduce.hip): an eighth of the bound
    "every survivor has min_cov instances or more", and 1024"""
    return n_reads * max(max_len - k + 1, 0) // max(min_cov, 1) // 8 + 1024


# ---- the read sets ----
NUC = "ACGT"


def rnd(rng, m):
    return "".join(NUC[b] for b in rng.integers(0, 4, m))


def synthetic_reads():
    """the `synthetic` fixture of tests/test_gpu_reduce_reads.py, draw for draw: a 2,000-base genome with a repeat and a SNP copy, reads of
    120..150 bases at depth 12 with 1 % substitutions, and a planted fork of 12 + 7 reads"""
    rng = np.random.default_rng(20240611)
    g = list(rnd(rng, 2000))
    g[1400:1460] = g[300:360]
    g[1700:1850] = g[700:850]
    g[1775] = NUC[(NUC.index(g[1775]) + 1) % 4]
    g = "".join(g)
    reads = []
    while sum(len(r) for r in reads) < 12 * len(g):
        n = int(rng.integers(120, 151))
        p = int(rng.integers(0, len(g) - n + 1))
        r = [NUC[(NUC.index(c) + 1 + int(rng.integers(0, 3))) % 4] if rng.random() < 0.01 else c for c in g[p:p + n]]
        reads.append("".join(r))
    s = rnd(rng, 150)
    v = s[:100] + NUC[(NUC.index(s[100]) + 2) % 4] + s[101:]
    return reads + [s] * 12 + [v] * 7


FORK_TAIL = 36


def forked_reads(tail=FORK_TAIL):
    """`synthetic` and behind it a second fork whose minor allele has three instances more that only short k-mers see: 12 x s, 7 x v (s with
    base 100 replaced) and three reads random(30) + v[tail:150] + random(30).  The k-mers over base 100 that lie inside v[tail:] are seen
    10 times, the longer ones 7 times: the fork is a variant at a short k (10 > 8), a variant at k >= 61 under E = 6 (7 > 6) and an error
    there under E = 8 (7 <= 8, 12 >= 1.5 * 7), so a long record's marker is no longer forced to -1 by the short side in the reduction"""
    rng = np.random.default_rng(7)
    s = rnd(rng, 150)
    v = s[:100] + NUC[(NUC.index(s[100]) + 2) % 4] + s[101:]
    extra = [rnd(rng, 30) + v[tail:150] + rnd(rng, 30) for _ in range(3)]
    return synthetic_reads() + [s] * 12 + [v] * 7 + extra


def doubled_reads():
    """64 random reads of 96..150 bases (the lengths drawn first), each present twice: every window survives min_cov = 2, so the counter's
    rows are many times the driver's first capacity and the second count runs at every k"""
    rng = np.random.default_rng(11)
    reads = [rnd(rng, int(n)) for n in rng.integers(96, 151, 64)]
    return [r for r in reads for _ in range(2)]


EDGES_LIST = (23, 31, 33, 65, 95)


def edges_reads():
    """reads of exactly k - 1, k, k + 1 and k + 2 bases for every k of EDGES_LIST and of 96 and 128 bases (a 32-base word edge), each
    twice, next to 40 reads of 100..150 bases drawn from a 400-base genome"""
    rng = np.random.default_rng(13)
    g = rnd(rng, 400)
    reads = []
    for _ in range(40):
        n = int(rng.integers(100, 151))
        p = int(rng.integers(0, len(g) - n + 1))
        reads.append(g[p:p + n])
    for n in sorted({k + d for k in EDGES_LIST for d in (-1, 0, 1, 2)} | {96, 128}):
        reads += [rnd(rng, n)] * 2
    return reads


def edge_read_lengths():
    return sorted({k + d for k in EDGES_LIST for d in (-1, 0, 1, 2)} | {96, 128})


def sensitive_reads():
    """the `planted_k31` reads of tests/golden/mercy_vectors.npz: stretches of single coverage between solid k-mers"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mercy_vectors.npz"))
    buf, off = bytes(z["planted_k31/reads"]), z["planted_k31/reads_off"]
    return [buf[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


READ_SETS = dict(forked=forked_reads, doubled=doubled_reads, edges=edges_reads, sensitive=sensitive_reads, none=lambda: [])
DEFAULT_LIST = (23, 31, 41, 53, 67, 81, 95)          # (the default list cut at 95)
E_LISTS = ((23, 67, 95), DEFAULT_LIST, (65, 81), (53, 67), (81, 95))
PARAM_LIST = (31, 41, 67)
PARAM_SETS = (dict(min_cov=3), dict(max_cov=11), dict(bubble=0), dict(front_clip=3, end_clip=5), dict(min_error_cov=5, min_repeat_fold=2.0))
DOUBLED_LIST = (23, 31, 41, 67, 95)
DOUBLED_ALL_LIST = (23, 31, 41)                      # (below 61: with min_cov = 1 every window is a row)


def _name(kw):
    return "_".join(f"{k}{v}" for k, v in kw.items()).replace(".", "p")


def cases():
    """every case the device is held to: name -> (read set, k list, parameters other than the defaults)"""
    out = {}
    for kl in E_LISTS:
        out["forked_k" + "_".join(map(str, kl)) + "_P8"] = ("forked", kl, dict(P=8))
    for P in (1, 3):
        out[f"forked_k23_67_95_P{P}"] = ("forked", (23, 67, 95), dict(P=P))
    for kw in PARAM_SETS:
        out["forked_" + _name(kw)] = ("forked", PARAM_LIST, dict(P=3, **kw))
    out["doubled"] = ("doubled", DOUBLED_LIST, dict(P=3))
    out["doubled_min_cov1"] = ("doubled", DOUBLED_ALL_LIST, dict(P=3, min_cov=1))
    out["edges"] = ("edges", EDGES_LIST, dict(P=3))
    out["sensitive"] = ("sensitive", (23, 31, 41), dict(P=8, sensitive=1))
    out["none"] = ("none", (23, 31, 41), dict())
    return out


def load_vectors(path):
    """tests/golden/reduce_reads_vectors.npz -> ({read set: reads}, {case: [text per k]}, {case: the counter's rows per k})"""
    z = np.load(path)

    def strings(key):
        b, off = z[key].tobytes().decode(), z[key + "_off"]
        return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    reads = {str(s): strings(f"reads/{s}") for s in z["sets"]}
    texts = {str(c): strings(f"{c}/texts") for c in z["names"]}
    rows = {str(c): [int(x) for x in z[f"{c}/rows"]] for c in z["names"]}
    return reads, texts, rows
