"""String model of the second contig fixing stage (P/ReflexivDSDynamicKmerFixingRoundTwo.java): test
infrastructure, imported by the tests and by tests/golden/make_fixing2_vectors.py only.

A record is (key, marker, ext, left, right) with key / ext ACGT strings, as in tests/fixing_model.py, whose loop pass -- the
model of the EXISTING dynamic-k pass -- this stage reuses unchanged.  A contig is (bases, left, right)."""
import os

import numpy as np

try:
    from tests import fixing_model as fm
    from tests import pymodel as pm
except ImportError:                                               # (the generator runs with tests/ itself on the path)
    import fixing_model as fm
    import pymodel as pm

MAX_ROUNDS = 29                                                    # `if (iterations >= 30) break` (:207)
END = 200                                                          # bases of a contig end (:278-279)
KEY = 30                                                           # the key of every record of 04Fixing: ONE long


def default_params(max_k, **kw):
    return fm.default_params(max_k, **kw)


def loop_rounds(p):
    """sort + loop rounds (:203-213): iterations 1 .. min(maximumIteration + 1, 29); -1 gives none"""
    return max(0, min(p["max_iteration"] + 1, MAX_ROUNDS))


def binarize(rows):
    """DynamicKmerBinarizerFromReducedToSubKmer (:562-752): the first stage's binarizer WITHOUT its length filter.  A key that
    is not 30 bases long, or a row without an extension, is refused (the stated deviation: the reference keeps nucleotideBinarySlot[0])"""
    out = fm.binarize(rows, dict(max_k=0))
    for r in out:
        if len(r[0]) != KEY or len(r[2]) < 1:
            raise ValueError("a key that is not 30 bases long, or a row without an extension")
    return out


def run_passes(recs, p, P, hits=None):
    """-> [(the sort's permutation, the loop's output partition starts, the record set behind the loop)] for every round"""
    out, cur = [], list(recs)
    for _ in range(loop_rounds(p)):
        perm = sorted(range(len(cur)), key=lambda i: pm.dyn_blocks(cur[i][0]))        # sort("k-1"): stable
        srt = [cur[i] for i in perm]
        assert srt == fm.sort_records(cur)
        cur, ost = fm.loop_pass(srt, pm.dyn_partition_starts(srt, P), p, hits)
        out.append((perm, ost, cur))
    return out


def pass_sources(srt, recs):
    """how the vectors store a loop pass: for every output record the index of the sorted input record it is (kept or flipped:
    the same contig, left and right), or -1 and the record in full where the loop merged"""
    where = {}
    for j, r in enumerate(srt):
        where.setdefault((fm.contig_of(r), r[3], r[4]), []).append(j)
    src, fresh = [], []
    for r in recs:
        cand = where.get((fm.contig_of(r), r[3], r[4]), [])
        if cand and len(r[0]) == KEY:
            src.append(cand.pop(0))
        else:
            src.append(-1)
            fresh.append(r)
    return src, fresh


def pass_from_sources(srt, src, markers, fresh):
    out, fresh = [], list(fresh)
    for j, m in zip(src, markers):
        if j < 0:
            out.append(fresh.pop(0))
            continue
        c, r = fm.contig_of(srt[j]), srt[j]
        out.append((c[:KEY], 1, c[KEY:], r[3], r[4]) if m == 1 else (c[len(c) - KEY:], 2, c[:len(c) - KEY], r[3], r[4]))
    return out


def contigs(recs, p):
    """DSBinaryFixingKmerWithLongExtensionToString (:293-560): key + extension for marker 1, extension + key otherwise; a contig
    shorter than 2 maxKmerSize is dropped.  TagStringContigRDDID's repeated length test (:999) selects nothing more"""
    out = []
    for rec in recs:
        c = fm.contig_of(rec)
        if len(c) >= 2 * p["max_k"]:
            out.append((c, rec[3], rec[4]))
    return out


def contig_id(c, idx):
    return f"Contig_{len(c[0])}_{c[1]}_{c[2]}_{idx}"


def to_text(cs):
    """zipWithIndex + TagStringContigRDDID (:987-1005): the rows of 05FixingAgain; idx = the position among the KEPT contigs"""
    return "".join(f"{contig_id(c, i)},{c[0]}\n" for i, c in enumerate(cs))


def ends_text(cs):
    """DSExtractContigEndsForAlignment (:265-291): the lines of 06ContigEnds"""
    out = []
    for i, c in enumerate(cs):
        s, name = c[0], contig_id(c, i)
        if len(s) >= 2 * END:
            out.append(f">{name}-L\n{s[:END]}\n>{name}-R\n{s[len(s) - END:]}\n")
        else:
            out.append(f">{name}\n{s}\n")
    return "".join(out)


def run_stages(rows, p, P, hits=None):
    """-> (the binarized records, [the record set behind every round], the kept contigs, 05FixingAgain, 06ContigEnds)"""
    recs = binarize(rows)
    passes = [x[2] for x in run_passes(recs, p, P, hits)]
    cs = contigs(passes[-1] if passes else recs, p)
    return recs, passes, cs, to_text(cs), ends_text(cs)


def run_text(rows, p, P):
    return run_stages(rows, p, P)[3:]


def load_case(z, name):
    """a case of tests/golden/fixing2_vectors.npz -> (params, P, rows, the binarized records, [(permutation of the round's sort,
    the loop's output partition starts, the records behind the loop)], text, ends text).  The file stores the rows (a case named fix_<name> reads the
    text of case <name> of fixing_vectors.npz instead), a sort as the
    permutation of the set before it, every loop pass as pass_sources gives it, and both texts."""
    v = z[name + "/meta"]
    p, P, rounds = dict(max_k=int(v[0]), scramble=int(v[1]), max_iteration=int(v[2])), int(v[3]), int(v[4])

    def strings(key):
        b, off = z[key].tobytes().decode(), z[key + "_off"]
        return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    if name.startswith("fix_"):                                    # the final text of that case of fixing_vectors.npz
        rows = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixing_vectors.npz"))[name[4:] + "/text"].tobytes().decode().splitlines()
    else:
        rows = [r.rstrip("\n") for r in strings(name + "/rows")]
    passes, prev = [], binarize(rows)
    for i in range(rounds):
        perm = [int(x) for x in z[f"{name}/sort{i}_perm"]]
        fresh = [(k, 1, e, int(a[0]), int(a[1])) for k, e, a in zip(strings(f"{name}/pass{i}_key"), strings(f"{name}/pass{i}_ext"), z[f"{name}/pass{i}_lr"])]
        markers = [int(x) for x in z[f"{name}/pass{i}_marker"]]
        k = 0
        for j, s in enumerate(z[f"{name}/pass{i}_src"]):           # (a record stored in full takes its marker from the marker array too)
            if s < 0:
                fresh[k] = (fresh[k][0], markers[j]) + fresh[k][2:]
                k += 1
        prev = pass_from_sources([prev[j] for j in perm], [int(x) for x in z[f"{name}/pass{i}_src"]], markers, fresh)
        passes.append((perm, [int(x) for x in z[f"{name}/pass{i}_ps"]], prev))
    return p, P, rows, binarize(rows), passes, z[name + "/text"].tobytes().decode(), z[name + "/ends"].tobytes().decode()
