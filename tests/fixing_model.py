"""String model of the contig fixing stage (P/ReflexivDSDynamicKmerFixing.java): test infrastructure,
imported by the tests and by tests/golden/make_fixing_vectors.py only.

A record is (key, marker, ext, left, right) with key / ext ACGT strings -- the form of pymodel's dynamic-k functions, whose
sort, partition cut and extend pass step 9 reuses unchanged.  `hits` (a dict) counts the branches the two folds and the
loop take."""
try:
    from tests import pymodel as pm
except ImportError:                                               # (the generator runs with tests/ itself on the path)
    import pymodel as pm

CLAMP = 30000
FIX_K = 31                                                         # FixedKmerSize, everywhere in the reference
STAGES = ("binarized", "long", "union", "sort1", "fold1", "reflected", "sort2", "fold2")
FOLD_BRANCHES = ("first", "long_replaces_short", "long_appended", "short_after_long_dropped", "short_replaces_short",
                 "short_larger_dropped", "short_new_key")
LOOP_BRANCHES = tuple(f"{side}: {what}" for side in ("forward row", "reflected row")
                      for what in ("both negative", "both non-negative", "own distance", "holder's distance", "no merge")) + \
    ("same marker", "unrelated", "flush")
_DECISIONS = set(LOOP_BRANCHES) - {"flush"}


def default_params(max_k, **kw):
    p = dict(max_k=max_k, scramble=2, max_iteration=150)
    p.update(kw)
    return p


def loop_rounds(p):
    """sort + loop rounds behind the unsorted first pass (:233-243): iterations 1 .. min(maximumIteration + 1, 17)"""
    return max(0, min(p["max_iteration"] + 1, 17))


def binarize(rows, p):
    """DynamicKmerBinarizerFromReducedToSubKmer (:3106-3203): 'SUBKMER,m|l|r,EXTENSION' (an optional leading '(' of the sub-k-mer,
    an optional trailing ')' of the attribute); a row of fewer than 2 max_k bases in all is dropped"""
    out = []
    for row in rows:
        key, attr, ext = row.rstrip("\r\n").split(",")
        if key.startswith("("):
            key = key[1:]
        if attr.endswith(")"):
            attr = attr[:-1]
        if len(key) + len(ext) < 2 * p["max_k"]:
            continue
        m, l, r = (int(x) for x in attr.split("|"))
        fix = lambda s: "".join(ch if ch in "ACG" else "T" for ch in s)     # noqa: E731
        out.append((fix(key), m, fix(ext), max(-CLAMP, min(CLAMP, l)), max(-CLAMP, min(CLAMP, r))))
    return out


def contig_of(rec):
    return rec[0] + rec[2] if rec[1] == 1 else rec[2] + rec[0]


def contig_ends(recs, p):
    """DSExtractFixingKmerFromContigEnds (:1190-1256) + DSgetFixingLongKmer (:520-541) / DSgetFixingKmer (:857-874):
    -> (the long records: the trimmed contigs cut key 30 / rest; the 31-mers in emission order)"""
    mk = p["max_k"]
    longs, kmers = [], []
    for rec in recs:
        c = contig_of(rec)
        L = len(c)
        if L < 2 * mk:
            continue
        for i in range(mk - FIX_K + 1):
            kmers.append(c[i:i + FIX_K])
            kmers.append(c[L - i - FIX_K:L - i])
        cut = mk - FIX_K + 1
        t = c[cut:L - cut]
        left = mk + 3 if rec[3] > 0 else rec[3]
        right = mk + 3 if rec[4] > 0 else rec[4]
        longs.append((t[:FIX_K - 1], 1, t[FIX_K - 1:], left, right))
    return longs, kmers


def kmer_set(kmers, longs, order=None):
    """groupBy("kmer").count() (the count is never read: distinct) + DSFixingKmerLeftAndRightMarkerAssignment (:1857-1878) +
    union (:213): the 31-mer records first.  order: None = first occurrence (Spark's is its hash order; nothing from the
    first fold on depends on it), "sorted" = ascending 2-bit value (the device's), or a permutation of the distinct set"""
    seen = list(dict.fromkeys(kmers))
    if order == "sorted":
        seen.sort()                                                # (A < C < G < T is the order of the 2-bit codes)
    elif order is not None:
        seen = [seen[i] for i in order]
    return [(k[:FIX_K - 1], 1, k[FIX_K - 1:], -1, -1) for k in seen] + list(longs)


def sort_records(recs):
    return pm.dyn_sort(recs)


def fold(recs, hits=None, tag="L"):
    """DSFilterForkSubKmerWithErrorCorrection (:2057-2116) / DSFilterForkReflectedSubKmerWithErrorCorrection (:2232-2283)
    over ONE partition: the two classes are the same text; the base compared is the extension's first"""
    out = []

    def hit(name):
        if hits is not None:
            hits[tag + " " + name] = hits.get(tag + " " + name, 0) + 1

    for s in recs:
        if not out:
            out.append(s); hit("first")
        elif len(s[2]) > 1:
            if s[0] == out[-1][0] and len(out[-1][2]) == 1:
                out[-1] = s; hit("long_replaces_short")
            else:
                out.append(s); hit("long_appended")
        elif s[0] == out[-1][0]:
            if len(out[-1][2]) > len(s[2]):
                hit("short_after_long_dropped")
            elif pm.NUC.index(s[2][0]) <= pm.NUC.index(out[-1][2][0]):
                out[-1] = s; hit("short_replaces_short")
            else:
                hit("short_larger_dropped")
        else:
            out.append(s); hit("short_new_key")
    return out


def fold_closed_form(recs):
    """the same fold over ONE partition, run by run: a run with a row longer than one base keeps exactly those rows, in
    order; any other run keeps its LAST row of the smallest base code (`<=` replaces)"""
    out, i = [], 0
    while i < len(recs):
        j = i
        while j < len(recs) and recs[j][0] == recs[i][0]:
            j += 1
        run = recs[i:j]
        longs = [r for r in run if len(r[2]) > 1]
        if longs:
            out += longs
        else:
            best = min(pm.NUC.index(r[2][0]) for r in run)
            out.append([r for r in run if pm.NUC.index(r[2][0]) == best][-1])
        i = j
    return out


def by_partition(fn, recs, P, starts=None):
    st = starts if starts is not None else pm.dyn_partition_starts(recs, P)
    out, ost = [], [0]
    for p in range(len(st) - 1):
        out += fn(recs[st[p]:st[p + 1]])
        ost.append(len(out))
    return out, st, ost


def reflect(recs):
    """DSChangingFixingKmerToReflectedKmer (:1571-1608): key = the LAST 30 bases, extension = the front, marker 2"""
    out = []
    for rec in recs:
        c = contig_of(rec)
        out.append((c[len(c) - (FIX_K - 1):], 2, c[:len(c) - (FIX_K - 1)], rec[3], rec[4]))
    return out


def loop_pass(recs, starts, p, hits=None):
    """DSExtendFixingKmerLoop (:2371-3104) over sorted records: every key has 30 bases, so it is the dynamic-k pass with no
    prefix relation (pymodel.dyn_extend_pass, stage 1 below iteration 61); the marker starts at 1 when scramble == 3"""
    out, ost, labels = pm.dyn_extend_pass(recs, starts, stage=1, start_iteration=5, start_marker=1 if p["scramble"] == 3 else 2)
    if hits is not None:
        dec = 0
        for lab in labels:
            if lab in _DECISIONS:
                hits[lab] = hits.get(lab, 0) + 1
                dec += 1
            elif lab.startswith("merge: bubble") or lab == "merge: ends inherited" or lab == "clamp":
                hits[lab] = hits.get(lab, 0) + 1
            else:
                raise AssertionError("the fixing loop took a branch of the dynamic-k pass it cannot reach: " + lab)
        hits["flush"] = hits.get("flush", 0) + len(out) - dec      # (every decision emits one row; the rest are flushes)
    return out, ost


def run_stages(rows, p, P, hits=None, order=None):
    """-> ({stage: records}, {stage: partition starts}, the 31-mers in emission order, [the record set behind every loop pass])"""
    st, ps = {}, {}
    st["binarized"] = binarize(rows, p)
    st["long"], kmers = contig_ends(st["binarized"], p)
    st["union"] = kmer_set(kmers, st["long"], order)
    st["sort1"] = sort_records(st["union"])
    st["fold1"], ps["sort1"], ps["fold1"] = by_partition(lambda r: fold(r, hits, "L"), st["sort1"], P)
    st["reflected"] = reflect(st["fold1"])
    st["sort2"] = sort_records(st["reflected"])
    st["fold2"], ps["sort2"], ps["fold2"] = by_partition(lambda r: fold(r, hits, "R"), st["sort2"], P)
    cur, _ = loop_pass(st["fold2"], ps["fold2"], p, hits)
    passes = [cur]
    for _ in range(loop_rounds(p)):
        cur = sort_records(cur)
        cur, _ = loop_pass(cur, pm.dyn_partition_starts(cur, P), p, hits)
        passes.append(cur)
    return st, ps, kmers, passes


def to_text(recs):
    """DSBinaryFixingKmerWithLongExtensionToString (:262-299)"""
    return "".join(f"{k},{m}|{l}|{r},{e}\n" for k, m, e, l, r in recs)


def from_text(text):
    out = []
    for row in text.splitlines():
        k, a, e = row.split(",")
        m, l, r = (int(x) for x in a.split("|"))
        out.append((k, m, e, l, r))
    return out


def run_text(rows, p, P):
    return to_text(run_stages(rows, p, P)[3][-1])


def load_case(z, name):
    """a case of tests/golden/fixing_vectors.npz -> (params, P, rows, {stage: records}, {stage: part starts}, 31-mers, passes,
    text).  The file stores the binarizer's output as the indices of the rows it keeps (their text IS the record), the union's
    31-mer records as indices into the 31-mers in emission order, a sort as the permutation of the stage before it, a fold as
    indices into its input, the last loop pass as the text, and every other stage as packed strings + attributes."""
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
    st["binarized"] = [binarize([rows[i]], p)[0] for i in z[name + "/binarized_rows"]]
    st["long"] = records("long")
    st["union"] = [kmer_set([kmers[i]], [])[0] for i in z[name + "/union_kmers"]] + st["long"]
    prev = st["union"]
    for s in STAGES[3:]:
        if f"{name}/{s}_perm" in z.files:
            st[s] = [prev[i] for i in z[f"{name}/{s}_perm"]]
        elif f"{name}/{s}_from" in z.files:
            st[s] = [prev[i] for i in z[f"{name}/{s}_from"]]
        else:
            st[s] = records(s)
        prev = st[s]
        if f"{name}/{s}_ps" in z.files:
            ps[s] = [int(x) for x in z[f"{name}/{s}_ps"]]
    passes = [records(f"pass{i}") for i in range(int(v[4]) - 1)] + [from_text(text)]
    return p, P, rows, st, ps, kmers, passes, text
