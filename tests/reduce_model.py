"""String model of the k-mer reduction stage (P/ReflexivDSDynamicKmerRuduction.java): test
infrastructure, imported by the tests and by tests/golden/make_reduce_vectors.py only.

A record is (key, ext, marker, left, right) with key / ext ACGT strings.  One call handles ONE pair k1 < k2: rows of
another length are dropped by the binarizer.  `hits` (a dict) counts the branches the two adjustments take."""
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
CLAMP = 30000
STAGES = ("union", "left_prep", "left_sort", "left_adj", "right_prep", "right_sort", "right_adj", "full", "full_sort", "neutral")


def supported_pair(k1, k2):
    """(the reference's classes of THIS stage are sound where k or k - 1 is a multiple of 31: `probe_k` of the vector file)"""
    return 8 <= k1 < k2 <= 124


def parse_rows(rows, ks):
    """DynamicKmerBinarizerFromSorted: 'KMER,m|l|r' (an optional leading '(' and trailing ')') -> full k-mer records"""
    out = []
    for row in rows:
        kmer, attr = row.rstrip("\r\n").split(",", 1)
        if kmer.startswith("("):
            kmer = kmer[1:]
        if attr.endswith(")"):
            attr = attr[:-1]
        if len(kmer) not in ks:
            continue
        m, l, r = (int(x) for x in attr.split("|"))
        kmer = "".join(ch if ch in "ACG" else "T" for ch in kmer)
        out.append((kmer, "", m, max(-CLAMP, min(CLAMP, l)), max(-CLAMP, min(CLAMP, r))))
    return out


def union(rows_short, rows_long, k1, k2):
    return parse_rows(rows_long, (k1, k2)) + parse_rows(rows_short, (k1, k2))


def left_prepare(recs):
    return [(k[:-1][::-1], k[-1], 1, l, r) for k, e, m, l, r in recs]


def right_prepare(recs):
    out = []
    for k, e, m, l, r in recs:
        c = k[::-1] + e if m == 1 else e + k[::-1]
        out.append((c[1:], c[0], 2, l, r))
    return out


def full_kmers(recs):
    return [((e + k) if m == 2 else (k + e), "", 1, l, r) for k, e, m, l, r in recs]


def block_key(key):
    """array<long> of 31-base blocks, the first base in the two highest bits, 01 behind the last base; signed"""
    out = []
    for j in range(0, max(len(key), 1), 31):
        chunk = key[j:j + 31]
        v = 0
        for i, ch in enumerate(chunk):
            v |= _CODE[ch] << (62 - 2 * i)
        if j + 31 >= len(key):
            v |= 1 << (62 - 2 * len(chunk))
        out.append(v - (1 << 64) if v >> 63 else v)
    return tuple(out)


def sort_records(recs):
    return sorted(recs, key=lambda r: block_key(r[0]))            # stable; tuples: element by element, a prefix first


def partition_starts(keys, P):
    n = len(keys)
    st, prev = [], 0
    for p in range(P):
        s = max(p * n // P, prev)
        while 0 < s < n and keys[s] == keys[s - 1]:
            s += 1
        st.append(s)
        prev = s
    st.append(n)
    return st


def prefix(a, b):
    """dynamicSubKmerComparator: the shorter one is a prefix of the longer one"""
    return b.startswith(a) if len(a) <= len(b) else a.startswith(b)


def adjust(recs, right, k1, hits=None):
    """LeftLongerKmerVariantAdjustment (right False) / RightLongerKmerVariantAdjustmentAndNeutralization (right True) over ONE
    partition, written as the reference writes it: two pending rows"""
    out = []
    tag = "R" if right else "L"

    def hit(name):
        if hits is not None:
            hits[tag + name] = hits.get(tag + name, 0) + 1

    def edit(t, s):
        k, e, m, l, r = t
        if right:
            l = -1 if s[3] < 0 <= l else l
        else:
            r = -1 if s[4] < 0 <= r else r
        return (k, s[1], m, l, r)

    S = lambda x: len(x[0]) == k1 - 1                             # noqa: E731
    P = lambda x, y: prefix(x[0], y[0])                           # noqa: E731
    a = b = None
    for c in recs:
        if a is None:
            a = c
            continue
        if b is None:
            b = c
            continue
        shape = "".join("S" if S(x) else "L" for x in (a, b, c))
        nxt, emit = None, None                                    # nxt: 'shift' | 'two' (a, b out, c pending) | 'three'
        if shape == "SSS":
            nxt, emit = "two", [a, b]; hit("SSS")
        elif shape == "SSL":
            if P(c, b):
                nxt = "shift"; hit("SSL_shift")
            else:
                nxt, emit = "two", [a, b]; hit("SSL_two")
        elif shape == "SLS":
            if P(b, a):
                nxt, emit = "two", ([edit(b, a)] if right else [a, edit(b, a)]); hit("SLS_edit")
            elif P(c, b):
                nxt = "shift"; hit("SLS_shift")
            else:
                nxt, emit = "two", [a, b]; hit("SLS_two")
        elif shape == "SLL":
            if P(b, a) and P(c, a):
                drop = right and (a[1] == b[1] or a[1] == c[1])
                nxt, emit = "three", ([b, c] if drop else [a, b, c]); hit("SLL_three_drop" if drop else "SLL_three")
            elif P(b, a):
                nxt, emit = "two", ([edit(b, a)] if right else [a, edit(b, a)]); hit("SLL_edit")
            else:
                nxt = "shift"; hit("SLL_shift")
        elif shape == "LSS":
            if P(a, b):
                nxt, emit = "two", ([edit(a, b)] if right else [edit(a, b), b]); hit("LSS_edit")
            else:
                nxt, emit = "two", [a, b]; hit("LSS_two")
        elif shape == "LSL":
            if P(a, b) and P(c, b):
                drop = right and (a[1] == b[1] or b[1] == c[1])
                nxt, emit = "three", ([a, c] if drop else [a, b, c]); hit("LSL_three_drop" if drop else "LSL_three")
            elif P(a, b):
                nxt, emit = "two", ([edit(a, b)] if right else [edit(a, b), b]); hit("LSL_edit")
            elif P(c, b):
                nxt = "shift"; hit("LSL_shift")
            else:
                nxt, emit = "two", [a, b]; hit("LSL_two")
        elif shape == "LLS":
            if P(a, c) and P(c, b):
                drop = right and (a[1] == c[1] or b[1] == c[1])
                nxt, emit = "three", ([a, b] if drop else [a, b, c]); hit("LLS_three_drop" if drop else "LLS_three")
            elif P(c, b):
                nxt = "shift"; hit("LLS_shift")
            else:
                nxt, emit = "two", [a, b]; hit("LLS_two")
        else:
            nxt = "shift"; hit("LLL")
        if nxt == "shift":
            out.append(a)
            a, b = b, c
        elif nxt == "two":
            out += emit
            a, b = c, None
        else:
            out += emit
            a = b = None
    if a is not None and b is not None:
        shape = ("S" if S(a) else "L") + ("S" if S(b) else "L")
        if shape == "SL" and P(a, b):
            out += [edit(b, a)] if right else [a, edit(b, a)]; hit("F_SL_edit")
        elif shape == "LS" and P(a, b):
            out += [edit(a, b)] if right else [edit(a, b), b]; hit("F_LS_edit")
        elif shape == "LS":
            hit("F_LS_none")                                       # the reference adds neither row
        else:
            out += [a, b]; hit("F_" + shape)
    elif a is not None:
        out.append(a); hit("F_one")
    return out


def neutralize(recs):
    """ShorterKmerNeutralization (the live code) over ONE partition"""
    out = []
    for c in recs:
        if not out or len(c[0]) == len(out[-1][0]) or not prefix(c[0], out[-1][0]):
            out.append(c)
        elif len(out[-1][0]) > len(c[0]):
            continue
        else:
            out[-1] = c
    return out


def by_partition(fn, recs, P, starts=None):
    st = starts if starts is not None else partition_starts([block_key(r[0]) for r in recs], P)
    out, ost = [], [0]
    for p in range(len(st) - 1):
        out += fn(recs[st[p]:st[p + 1]])
        ost.append(len(out))
    return out, st, ost


def to_text(recs, k):
    return "".join(f"{key},{m}|{l}|{r}\n" for key, e, m, l, r in recs if len(key) == k)


def run_stages(rows_short, rows_long, k1, k2, P, hits=None):
    """every stage's record set by name, and the partition starts going into / coming out of the partitioned operators"""
    st, ps = {}, {}
    st["union"] = union(rows_short, rows_long, k1, k2)
    st["left_prep"] = left_prepare(st["union"])
    st["left_sort"] = sort_records(st["left_prep"])
    st["left_adj"], ps["left_sort"], ps["left_adj"] = by_partition(lambda r: adjust(r, False, k1, hits), st["left_sort"], P)
    st["right_prep"] = right_prepare(st["left_adj"])
    st["right_sort"] = sort_records(st["right_prep"])
    st["right_adj"], ps["right_sort"], ps["right_adj"] = by_partition(lambda r: adjust(r, True, k1, hits), st["right_sort"], P)
    st["full"] = full_kmers(st["right_adj"])
    st["full_sort"] = sort_records(st["full"])
    st["neutral"], ps["full_sort"], ps["neutral"] = by_partition(neutralize, st["full_sort"], P)
    return st, ps


def run_text(rows_short, rows_long, k1, k2, P):
    st, _ = run_stages(rows_short, rows_long, k1, k2, P)
    return to_text(st["neutral"], k1), to_text(st["neutral"], k2)


def handover(text):
    """what rfx_dyn_binarize form 0 makes of the stage's text"""
    out = []
    for row in text.splitlines():
        kmer, attr = row.split(",")
        m, l, r = (int(x) for x in attr.split("|"))
        out.append((kmer[:-1], kmer[-1], 1, l, r))
    return out


def load_case(z, name):
    """a case of tests/golden/reduce_vectors.npz -> (meta dict, short rows, long rows, {stage: records}, {stage: part starts},
    text of k1, text of k2).  The file stores a sort as the permutation of the stage before it, an adjustment's / the
    neutralizer's output as indices into its input plus the (possibly edited) extension and attributes, and a twin case
    (the same rows under another max_k) names the case whose sequences it shares."""
    v = z[name + "/meta"]
    meta = dict(k1=int(v[0]), k2=int(v[1]), max_k=int(v[2]), P=int(v[3]))
    src = str(z[name + "/seqs_from"]) if name + "/seqs_from" in z.files else name

    def strings(key):
        b, off = z[key].tobytes().decode(), z[key + "_off"]
        return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    rows_s, rows_l = strings(src + "/rows_short"), strings(src + "/rows_long")
    st, ps, prev = {}, {}, None
    for s in STAGES:
        mlr = z[f"{src}/{s}_mlr"]
        if f"{src}/{s}_perm" in z.files:
            seqs = [prev[i][:2] for i in z[f"{src}/{s}_perm"]]
        elif f"{src}/{s}_from" in z.files:
            ext = z[f"{src}/{s}_ext"].tobytes().decode()
            seqs = [(prev[i][0], ext[j] if ext else "") for j, i in enumerate(z[f"{src}/{s}_from"])]
        else:
            ext = z[f"{src}/{s}_ext"].tobytes().decode()
            seqs = [(k, ext[j] if ext else "") for j, k in enumerate(strings(f"{src}/{s}_key"))]
        st[s] = prev = [(a, b, int(m), int(l), int(r)) for (a, b), (m, l, r) in zip(seqs, mlr)]
        if f"{src}/{s}_ps" in z.files:
            ps[s] = [int(x) for x in z[f"{src}/{s}_ps"]]
    return meta, rows_s, rows_l, st, ps, z[src + "/text1"].tobytes().decode(), z[src + "/text2"].tobytes().decode()
