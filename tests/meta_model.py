"""The whole call from reads to contigs (rfx_dev_meta_reads / rfx_meta_reads) as strings, joined from the models
that exist -- tests/reduce_reads_model.py, the oracle's first-four passes and iterations (per job, with the job's own start), the
string models of 04Fixing, 05FixingAgain / 06ContigEnds, the end mapping, 07EndExtend, 08Extend and 09ExtendAgain, and the oracle's
contig de-duplication -- with the orchestrator's partition rule written from Pipelines.java (:877-883, :914-921, :954-974).  Every
stage hands the next one its TEXT, as the reference's stages hand over files.  Test infrastructure: it shares no code with the
library.  The read sets of the tests are here too, and tests/golden/make_meta_vectors.py stores them with every stage's text."""
import numpy as np

from oracle import oracle as O
from tests import endext_model as E
from tests import extend_model as X
from tests import fixing2_model as F2
from tests import fixing_model as F
from tests import map_model as M
from tests import reduce_reads_model as RR

JOBS = ((5, 9), (10, 14), (15, 19), (21, 30), (31, 40), (41, 50), (51, 60), (61, 70))      # :886, :925: there is no iteration 20
STAGES = ("00firstFour",) + tuple(f"01Iteration{a}_{b}" for a, b in JOBS) + ("04Fixing", "05FixingAgain", "06ContigEnds", "Mapping", "07EndExtend",
                                                                              "08Extend", "09ExtendAgain", "Assembly")
DEFAULTS = dict(scramble=2, max_iteration=150, min_contig=500, seed=21, min_overlap=31, max_mismatch=2)


def p_rule(O_):
    """Pipelines.java: `if (OriginalPartition >= 10) param.partitions = OriginalPartition * 80 / 100` ahead of the iterations 5-19
    (:877-883), `* 60 / 100` ahead of 21-70 (:914-921), and ahead of the fixing stage and every stage behind it `* 10 / 100` from 1000,
    `* 20 / 100` from 100, else `* 40 / 100` (:954-974); Java int arithmetic -> (first four, 5-19, 21-70, the later stages)"""
    if O_ < 10:
        return O_, O_, O_, O_
    late = O_ * 10 // 100 if O_ >= 1000 else O_ * 20 // 100 if O_ >= 100 else O_ * 40 // 100
    return O_, O_ * 80 // 100, O_ * 60 // 100, late


def same_p(O_):
    """the caller's P throughout: what a user gets who forgets the rule"""
    return O_, O_, O_, O_


def lines(text):
    return text.splitlines(keepends=True)


def dyn_text(rows):
    return "".join(f"{k},{a},{e}\n" for k, a, e in rows)


def run(reads, klist, O_, rule=p_rule, last_job_start=61, reduce_params=None, **params):
    """-> ({stage: its file's text}, {stage: the records or contigs it leaves; "reduced", "hits"}).  last_job_start = 51 runs the job
    61-70 under the rule of the iterations below 61 (what skipping the >= 61 rule means)"""
    prm = dict(DEFAULTS, **params)
    max_k = int(klist[-1])
    P0, P1, P2, P3 = rule(O_)
    fp = F.default_params(max_k, scramble=prm["scramble"], max_iteration=prm["max_iteration"])
    text, count = {}, {}
    if not reads:
        return {s: "" for s in STAGES}, dict({s: 0 for s in STAGES}, reduced=0, hits=0)
    reduced = RR.model(reads, klist, **dict(reduce_params or {}))
    rows = [tuple(r.rstrip("\n").split(",")) for t in reduced for r in lines(t)]
    count["reduced"] = len(rows)
    cur, _ = O.dyn_first_four(rows, P0)
    text["00firstFour"], count["00firstFour"] = dyn_text(cur), len(cur)
    for (a, b), P in zip(JOBS, (P1, P1, P1, P2, P2, P2, P2, P2)):
        start = last_job_start if a == 61 else a
        cur, _ = O.dyn_iterations(cur, P, start, start + (b - a)) if cur else ([], None)
        name = f"01Iteration{a}_{b}"
        text[name], count[name] = dyn_text(cur), len(cur)
    t = text["01Iteration61_70"]
    text["04Fixing"] = F.run_text(lines(t), fp, P3)
    text["05FixingAgain"], text["06ContigEnds"] = F2.run_text(lines(text["04Fixing"]), fp, P3)
    contigs = E.contigs_of_text(text["05FixingAgain"])
    hits = M.rows(contigs, reads, seed=prm["seed"], min_overlap=prm["min_overlap"], max_mismatch=prm["max_mismatch"])
    text["Mapping"] = "".join(r + "\n" for r in hits)
    text["07EndExtend"] = E.run_text(text["05FixingAgain"], hits, max_k)
    text["08Extend"] = X.run_text(lines(text["07EndExtend"]), fp, P3)
    text["09ExtendAgain"] = X.run2_text(lines(text["08Extend"]), fp, P3)
    final = [r.rstrip("\n").split(",")[1] for r in lines(text["09ExtendAgain"])]
    dd = O.dedup_contigs(final, prm["min_contig"])
    text["Assembly"] = dd["text"]
    for s in ("04Fixing", "05FixingAgain", "Mapping", "07EndExtend", "08Extend", "09ExtendAgain"):
        count[s] = text[s].count("\n")
    count["06ContigEnds"], count["hits"], count["Assembly"] = count["05FixingAgain"], count["Mapping"], len(dd["rounds"][-1])
    return text, count


# ---- the read sets -----------------------------------------------------------------------------------------------------------------
def planted_reads(seed, genome_len=3000, read_lens=(100, 150), depth=24):
    """a planted genome with a fork (a segment continued in two ways, the second way at the genome's end) and one reverse-complemented
    repeat, reads of 100..150 bases on both strands, error free, at about `depth` -> the reads (fewer than 1,000)"""
    rng = np.random.default_rng(seed)
    g = M.rand_seq(rng, genome_len)
    stem = g[700:860]
    g = g[:genome_len - 300] + stem + M.rand_seq(rng, 140)                                   # the fork: stem + another continuation
    g = g[:1500] + M.revcomp(g[300:420]) + g[1620:]                                          # the repeat, reverse-complemented
    n = depth * len(g) // ((read_lens[0] + read_lens[1]) // 2)
    reads = []
    for i in range(n):
        L = int(rng.integers(read_lens[0], read_lens[1] + 1))
        at = int(rng.integers(0, len(g) - L + 1))
        r = g[at:at + L]
        reads.append(M.revcomp(r) if i % 2 else r)
    assert len(reads) < 1000
    return reads


def cases():
    """name -> (reads, klist, O, reduce params, params)"""
    reads = planted_reads(7)
    small = dict(min_contig=100)
    return {
        "k23_31_41_O8": (reads, (23, 31, 41), 8, dict(P=8), small),
        "k23_31_41_O10": (reads, (23, 31, 41), 10, dict(P=10), small),
        "k23_67_95_O10": (planted_reads(11, depth=28), (23, 67, 95), 10, dict(P=10), small),
    }


# ---- the vector file (tests/golden/meta_vectors.npz) -----------------------------------------------------------------------------------
def facts(name, reads, klist, O_, rp, p, text):
    """what test_meta_model.py asserts of a case, measured on the model: the first stage at which P = O throughout gives another text
    (O >= 10 only), and the first stage that changes when the job 61-70 runs under the rule of the iterations below 61"""
    out = {}
    if O_ >= 10:
        same, _ = run(reads, klist, O_, rule=same_p, reduce_params=rp, **p)
        out["rule_stage"] = next((s for s in STAGES if same[s] != text[s]), "")
    skip, _ = run(reads, klist, O_, last_job_start=51, reduce_params=rp, **p)
    out["skip61_stage"] = next((s for s in STAGES if skip[s] != text[s]), "")
    return out


def build_vectors():
    """-> the arrays of the vector file: per case the reads (bytes + offsets), the k list, O, the parameters, every stage's text, the
    counts and the facts"""
    z = {"names": np.array(list(cases()))}
    for name, (reads, klist, O_, rp, p) in cases().items():
        text, count = run(reads, klist, O_, reduce_params=rp, **p)
        off = np.zeros(len(reads) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in reads])
        z[f"{name}/reads"] = np.frombuffer("".join(reads).encode(), np.uint8)
        z[f"{name}/read_off"] = off
        z[f"{name}/klist"] = np.array(klist, np.int32)
        z[f"{name}/meta"] = np.array([O_, rp["P"], p["min_contig"]], np.int32)
        for s in STAGES:
            z[f"{name}/text/{s}"] = np.frombuffer(text[s].encode(), np.uint8)
        z[f"{name}/counts"] = np.array([count[s] for s in STAGES] + [count["reduced"], count["hits"]], np.int64)
        for k, v in facts(name, reads, klist, O_, rp, p, text).items():
            z[f"{name}/{k}"] = np.frombuffer(v.encode(), np.uint8)
    return z


def load_vectors(path):
    """name -> (reads, klist, O, reduce params, params, {stage: text}, {stage: count, "reduced", "hits"}, {fact: stage name})"""
    z = np.load(path)
    out = {}
    for name in (str(x) for x in z["names"]):
        b, off = z[f"{name}/reads"].tobytes().decode(), z[f"{name}/read_off"]
        reads = [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
        O_, rp_P, min_contig = (int(x) for x in z[f"{name}/meta"])
        text = {s: z[f"{name}/text/{s}"].tobytes().decode() for s in STAGES}
        c = z[f"{name}/counts"]
        count = dict({s: int(c[i]) for i, s in enumerate(STAGES)}, reduced=int(c[len(STAGES)]), hits=int(c[len(STAGES) + 1]))
        fx = {k: z[f"{name}/{k}"].tobytes().decode() for k in ("rule_stage", "skip61_stage") if f"{name}/{k}" in z.files}
        out[name] = (reads, tuple(int(k) for k in z[f"{name}/klist"]), O_, dict(P=rp_P), dict(min_contig=min_contig), text, count, fx)
    return out
