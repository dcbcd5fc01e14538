"""String model of the contig extension stages (P/ReflexivDSDynamicKmerExtend.java and P/ReflexivDSDynamicKmerExtendRoundTwo.java,
DESIGN.md section 25): test infrastructure, imported by the tests and by tests/golden/make_extend_vectors.py only.

08Extend is the contig fixing stage with another binarizer and other contig ends: only those two steps are here, everything behind
them is tests/fixing_model.py, unchanged.  09ExtendAgain is tests/fixing2_model.py behind another row header.  A record is (key,
marker, ext, left, right) as there; a binarized row carries (ll, rl) behind it."""
import os

import numpy as np

try:
    from tests import fixing_model as fm
    from tests import fixing2_model as f2
    from tests import pymodel as pm
except ImportError:                                               # (the generator runs with tests/ itself on the path)
    import fixing_model as fm
    import fixing2_model as f2
    import pymodel as pm

FIX_K = fm.FIX_K
CLAMP = fm.CLAMP
LONGEST = 303                                                      # characters of a consensus end: 300 bases and a literal
MIN_CUT = 32                                                       # deviation 1: a shorter cut contig is refused
STAGES = fm.STAGES
LINE_MAX = 10_000_000                                              # deviation 3: 09's text refuses a contig that long


def default_params(max_k, **kw):
    return fm.default_params(max_k, **kw)


def loop_rounds(p):
    return fm.loop_rounds(p)


def clamp(v):
    return max(-CLAMP, min(CLAMP, v))


def fix(s):
    """nucleotideValue: every character other than A, C and G reads as T"""
    return "".join(ch if ch in "ACG" else "T" for ch in s)


def parse_row(row):
    """a row of 07EndExtend -> ([L, left, right, idx, ll, rl, new], sequence).  ValueError: what rfx_dev_ext_from_text refuses -- an
    ID that is not '>Contig_' and seven decimal ints, a sequence that starts with '('"""
    row = row.rstrip("\r\n")
    ident, sep, seq = row.partition(",")
    if not sep or not ident.startswith(">Contig_"):
        raise ValueError("no >Contig_ ID and a comma: " + row[:60])
    f = ident[len(">Contig_"):].split("_")
    if len(f) != 7:
        raise ValueError("not seven fields: " + ident)
    vals = []
    for x in f:
        d = x[1:] if x[:1] in "+-" else x
        if not d.isdigit() or not d.isascii() or len(d) > 10 or not -2 ** 31 <= int(x) < 2 ** 31:
            raise ValueError("no decimal int: " + ident)
        vals.append(int(x))
    if seq.startswith("("):
        raise ValueError("a sequence that starts with '('")
    return vals, seq


def binarize(rows, p):
    """DynamicKmerBinarizerFromReducedToSubKmer (:3118-3219): key = the first 31 characters, extension = the rest, a row of fewer than
    2 max_k characters dropped, attribute (1, left, right) and a fourth column (1, ll, rl) -> [(key, 1, ext, left, right, ll, rl)]"""
    out = []
    for row in rows:
        (_, left, right, _, ll, rl, _), seq = parse_row(row)
        if len(seq) < 2 * p["max_k"]:
            continue
        out.append((fix(seq[:FIX_K]), 1, fix(seq[FIX_K:]), clamp(left), clamp(right), clamp(ll), clamp(rl)))
    return out


def check_ends(T, ll, rl):
    """what rfx_dev_ext_contig_ends refuses of a kept contig: end lengths no consensus has, and deviation 1"""
    if not (0 <= ll <= LONGEST and 0 <= rl <= LONGEST):
        raise ValueError("an end length outside 0..303")
    if T - ll - rl < MIN_CUT:
        raise ValueError("a cut contig of fewer than 32 characters")


def contig_ends(recs, p):
    """DSExtractFixingKmerFromContigEnds (:1189-1267) + DSgetFixingLongKmer / DSgetFixingKmer: -> (the long records: the cut contigs
    [ll, T - rl) cut key 30 / rest, left and right kept; the 31-mers in emission order)"""
    longs, kmers = [], []
    for key, _, ext, left, right, ll, rl in recs:
        c = key + ext
        T = len(c)
        if T < 2 * p["max_k"]:
            continue
        check_ends(T, ll, rl)
        for i in range(ll):
            kmers.append(c[i:i + FIX_K])
        for i in range(rl - 1, -1, -1):
            kmers.append(c[T - i - FIX_K:T - i])
        cut = c[ll:T - rl]
        longs.append((cut[:FIX_K - 1], 1, cut[FIX_K - 1:], left, right))
    return longs, kmers


def from_ends(longs, kmers, p, P, hits=None, order=None, st=None, ps=None):
    """steps 3-9, every one of them the fixing model's -> ({stage: records}, {stage: partition starts}, [the set behind every loop pass])"""
    st = {} if st is None else st
    ps = {} if ps is None else ps
    st["long"] = longs
    st["union"] = fm.kmer_set(kmers, longs, order)
    st["sort1"] = fm.sort_records(st["union"])
    st["fold1"], ps["sort1"], ps["fold1"] = fm.by_partition(lambda r: fm.fold(r, hits, "L"), st["sort1"], P)
    st["reflected"] = fm.reflect(st["fold1"])
    st["sort2"] = fm.sort_records(st["reflected"])
    st["fold2"], ps["sort2"], ps["fold2"] = fm.by_partition(lambda r: fm.fold(r, hits, "R"), st["sort2"], P)
    cur, _ = fm.loop_pass(st["fold2"], ps["fold2"], p, hits)
    passes = [cur]
    for _ in range(loop_rounds(p)):
        cur = fm.sort_records(cur)
        cur, _ = fm.loop_pass(cur, pm.dyn_partition_starts(cur, P), p, hits)
        passes.append(cur)
    return st, ps, passes


def run_stages(rows, p, P, hits=None, order=None):
    """-> ({stage: records}, {stage: partition starts}, the 31-mers in emission order, [the record set behind every loop pass]);
    stage "binarized" holds the seven-field rows"""
    st = {"binarized": binarize(rows, p)}
    longs, kmers = contig_ends(st["binarized"], p)
    st, ps, passes = from_ends(longs, kmers, p, P, hits, order, st)
    return st, ps, kmers, passes


def to_text(recs):
    return fm.to_text(recs)


def run_text(rows, p, P):
    return to_text(run_stages(rows, p, P)[3][-1])


# ---- the device's view: bases without the literals, and flags -------------------------------------------------------------------------
def device_set(rows, p, literals_in_flags=True):
    """the rows of 07EndExtend -> what rfx_dev_endext_contigs leaves of them (literals_in_flags) or what rfx_dev_ext_from_text makes of
    them (the literals as T bases, flags 0): [{bases, left, right, left_len, right_len, flags, src_idx, new_idx}] of the rows of at least
    2 max_k characters"""
    out = []
    for row in rows:
        (_, left, right, idx, ll, rl, new), seq = parse_row(row)
        if len(seq) < 2 * p["max_k"]:
            continue
        T, f = len(seq), 0
        if literals_in_flags:
            if ll >= 3 and seq[ll - 3:ll] == "-1l":
                f |= 1
            if rl >= 3 and seq[T - rl:T - rl + 3] == "r1-":
                f |= 2
        bases = seq
        if f & 2:
            bases = bases[:T - rl] + bases[T - rl + 3:]
        if f & 1:
            bases = bases[:ll - 3] + bases[ll:]
        out.append(dict(bases=fix(bases), left=left, right=right, left_len=ll, right_len=rl, flags=f, src_idx=idx, new_idx=new))
    return out


def set_text_chars(c):
    """the characters the stage reads of a contig of the device's set: three T per flagged seam"""
    b, ll, rl, f = c["bases"], c["left_len"], c["right_len"], c["flags"]
    if f & 1:
        b = b[:ll - 3] + "TTT" + b[ll - 3:]
    if f & 2:
        T = len(b) + 3
        b = b[:T - rl] + "TTT" + b[T - rl:]
    return b


def set_contig_ends(cs, p):
    """contig_ends on the device's set"""
    recs = []
    for c in cs:
        if not 0 <= c["flags"] <= 3 or c["left_len"] < 3 * (c["flags"] & 1) or c["right_len"] < 3 * (c["flags"] >> 1):
            raise ValueError("flags outside 0..3, or a flagged side of fewer than 3 characters")
        s = set_text_chars(c)
        recs.append((s[:FIX_K], 1, s[FIX_K:], clamp(c["left"]), clamp(c["right"]), c["left_len"], c["right_len"]))
    return contig_ends(recs, p)


def seam_overlaps(cs, p):
    """{(side, characters of the seam inside a 31-mer's window)} over every end 31-mer of the set: what the generator asks for"""
    seen = set()
    for c in cs:
        T = len(c["bases"]) + 3 * (c["flags"] & 1) + 3 * (c["flags"] >> 1)
        if T < 2 * p["max_k"]:
            continue
        ll, rl = c["left_len"], c["right_len"]
        starts = list(range(ll)) + [T - i - FIX_K for i in range(rl - 1, -1, -1)]
        for side, s in (("L", ll - 3 if c["flags"] & 1 else None), ("R", T - rl if c["flags"] & 2 else None)):
            if s is None:
                continue
            for q in starts:
                n = min(q + FIX_K, s + 3) - max(q, s)
                if n > 0:
                    seen.add((side, n))
    return seen


# ---- 09ExtendAgain ------------------------------------------------------------------------------------------------------------------
def to_text2(cs):
    """zipWithIndex + TagRowContigRDDID (ExtendRoundTwo :674-692) over the contigs DSBinaryFixingKmerToFullKmer (:415-456) keeps"""
    for c in cs:
        if len(c[0]) >= LINE_MAX:
            raise ValueError("a contig of 10,000,000 bases or more")
    return "".join(f">Contig-{len(c[0])}-{i},{c[0]}\n" for i, c in enumerate(cs))


def run2_stages(rows, p, P, hits=None):
    """the rows of 08Extend -> (the binarized records, [(permutation, partition starts, records)] per round, the kept contigs, text)"""
    recs = f2.binarize(rows)
    passes = f2.run_passes(recs, p, P, hits)
    cs = f2.contigs(passes[-1][2] if passes else recs, p)
    return recs, passes, cs, to_text2(cs)


def run2_text(rows, p, P):
    return run2_stages(rows, p, P)[3]


# ---- the vector file ------------------------------------------------------------------------------------------------------------------
def get_pass(z, tag, srt):
    """a stored loop pass over its input `srt` (fixing2_model.pass_sources: the index of the source and the marker of a record the loop
    passed on or flipped, a merged record in full) -> the records"""
    b = {k: z[f"{tag}_{k}"].tobytes().decode() for k in ("key", "ext")}
    off = {k: z[f"{tag}_{k}_off"] for k in ("key", "ext")}
    markers = [int(x) for x in z[tag + "_marker"]]
    src = [int(x) for x in z[tag + "_src"]]
    full = [j for j, s in enumerate(src) if s < 0]
    fresh = [(b["key"][off["key"][i]:off["key"][i + 1]], markers[j], b["ext"][off["ext"][i]:off["ext"][i + 1]], int(a[0]), int(a[1]))
             for i, (j, a) in enumerate(zip(full, z[tag + "_lr"]))]
    return f2.pass_from_sources(srt, src, markers, fresh)


def load_case(z, name):
    """a case of tests/golden/extend_vectors.npz -> (params, P, rows, {stage: records}, {stage: part starts}, 31-mers, passes, text, the
    rounds of 09 [(permutation, partition starts, records)], the text of 09).  Stored as fixing_vectors.npz and fixing2_vectors.npz
    store theirs: the binarizer's output is the model's of the rows, the union's 31-mer records indices into the 31-mers in emission
    order, a sort a permutation, a fold indices into its input, the last loop pass the text, every other loop pass of 08 and every round
    of 09 as fixing2_model.pass_sources gives it."""
    v = z[name + "/meta"]
    p, P = dict(max_k=int(v[0]), scramble=int(v[1]), max_iteration=int(v[2])), int(v[3])

    def strings(key):
        b, off = z[key].tobytes().decode(), z[key + "_off"]
        return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    def records(tag):
        mlr = z[f"{name}/{tag}_mlr"]
        return [(k, int(a[0]), e, int(a[1]), int(a[2])) for k, e, a in zip(strings(f"{name}/{tag}_key"), strings(f"{name}/{tag}_ext"), mlr)]

    rows = [r.rstrip("\n") for r in strings(name + "/rows")]
    kmers = strings(name + "/kmers")
    text = z[name + "/text"].tobytes().decode()
    st, ps = {}, {}
    st["binarized"] = binarize(rows, p)
    st["long"] = records("long")
    st["union"] = [fm.kmer_set([kmers[i]], [])[0] for i in z[name + "/union_kmers"]] + st["long"]
    prev = st["union"]
    for s in STAGES[3:]:
        if f"{name}/{s}_perm" in z.files:
            st[s] = [prev[i] for i in z[f"{name}/{s}_perm"]]
        elif f"{name}/{s}_from" in z.files:
            st[s] = [prev[i] for i in z[f"{name}/{s}_from"]]
        else:                                                      # (the reflection, stored as a pass over its input)
            st[s] = get_pass(z, f"{name}/{s}", prev)
        prev = st[s]
        if f"{name}/{s}_ps" in z.files:
            ps[s] = [int(x) for x in z[f"{name}/{s}_ps"]]
    passes, prev = [], st["fold2"]
    for i in range(int(v[4]) - 1):                                 # (the first pass runs on the fold's order, the others behind a sort)
        prev = get_pass(z, f"{name}/pass{i}", prev if i == 0 else fm.sort_records(prev))
        passes.append(prev)
    passes.append(fm.from_text(text))
    rounds2, prev = [], f2.binarize(text.splitlines())
    for i in range(int(v[5])):
        tag = f"{name}/x2_"
        perm = [int(x) for x in z[f"{tag}sort{i}_perm"]]
        prev = get_pass(z, f"{tag}pass{i}", [prev[j] for j in perm])
        rounds2.append((perm, [int(x) for x in z[f"{tag}pass{i}_ps"]], prev))
    return p, P, rows, st, ps, kmers, passes, text, rounds2, z[name + "/text2"].tobytes().decode()


VEC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extend_vectors.npz")


def case_names():
    return [str(x) for x in np.load(VEC)["names"]]
