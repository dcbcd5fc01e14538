"""String model of the k-mer sorting stage (P/ReflexivDSKmerLeftAndRightSorting.java): test
infrastructure, imported by the tests and by tests/golden/make_ksort_vectors.py only.

A record is (key, ext, marker, left, right) with key / ext ACGT strings.  One call handles ONE k: rows of another length
are dropped by the binarizer."""
COMP = str.maketrans("ACGT", "TGCA")
CLAMP = 30000
_SIGNED = {"G": 0, "T": 1, "A": 2, "C": 3}        # a base in the two highest bits of a signed long: G < T < A < C
_PLAIN = {"A": 0, "C": 1, "G": 2, "T": 3}


class BadRow(ValueError):
    """what the device answers with RFX_E_ARG"""


def default_params(k, **kw):
    p = dict(k=k, max_k=95, min_error_cov=8, max_cov=10000000, bubble=1, min_repeat_fold=1.5)
    p.update(kw)
    return p


def supported_k(k):
    return 8 <= k <= 124 and (k - 1) % 31 != 0


def parse_row(row):
    """-> (k-mer with every letter that is not ACG read as T, count)"""
    row = row.rstrip("\r\n")
    if "," not in row:
        raise BadRow("no comma")
    kmer, count = row.split(",", 1)
    if kmer.startswith("("):
        kmer = kmer[1:]
    if count.endswith(")"):
        count = count[:-1]
    if not count or not all("0" <= c <= "9" for c in count):
        raise BadRow("count")
    c = 1000000000 if len(count) >= 10 else int(count)
    return "".join(ch if ch in "ACG" else "T" for ch in kmer), c


def binarize(rows, p):
    """steps 1-4: two records per kept row, the k-mer's and then its reverse complement's"""
    out = []
    for row in rows:
        kmer, c = parse_row(row)
        if len(kmer) != p["k"] or c > p["max_cov"]:
            continue
        c = min(c, CLAMP)
        for s in (kmer, kmer.translate(COMP)[::-1]):
            out.append((s[:-1], s[-1], 1, c, c))
    return out


def _block_key(key):
    """sort("k-1"): array<long> element by element as signed longs; the first base of every 31-base block carries the sign"""
    return tuple(_SIGNED[b] if j % 31 == 0 else _PLAIN[b] for j, b in enumerate(key))


def sort_records(recs):
    return sorted(recs, key=lambda r: _block_key(r[0]))          # stable


def fork_filter(recs, reflected, p):
    E, F, M = p["min_error_cov"], float(p["min_repeat_fold"]), p["max_k"] + 3
    out = []
    key = None
    for k_, ext, marker, left, right in recs:
        if k_ != key:
            if key is not None:
                out.append((key, S[0], mk, S[1], S[2]))
            key, mk = k_, marker
            if reflected:
                H, S = left, [ext, -1, right]
            else:
                S = [ext, left, -1]
            continue
        if not reflected:
            hi = S[1]
            x = -1 if hi == 1 else M
            if left > hi:
                S = [ext, left, -1 if (hi <= E and left >= F * hi) else x]
            elif left == hi:
                if _SIGNED[ext] > _SIGNED[S[0]]:
                    S = [ext, left, x]
                else:
                    S[2] = x
            elif left <= E and hi >= F * left:
                S[2] = -1
            else:
                S[1], S[2] = left, (-1 if left == 1 else M)
        else:
            if left > H:
                S = [ext, -1 if (H <= E and left >= F * H) else M, right]
                H = left
            elif left == H:
                if _PLAIN[ext] > _PLAIN[S[0]]:
                    S = [ext, M, -1 if H == 1 else right]
                else:
                    S[1] = M
            elif left <= E and H >= F * left:
                S[1] = -1
            else:
                S[1], S[2] = M, (-1 if left == 1 else right)
    if key is not None:
        out.append((key, S[0], mk, S[1], S[2]))
    return out


def reflect(recs):
    """step 6"""
    return [(k[1:] + e, k[0], 2, l, r) for k, e, m, l, r in recs]


def full_kmers(recs):
    """step 8"""
    return [((e + k) if m == 2 else (k + e), "", 1, l, r) for k, e, m, l, r in recs]


def to_text(recs, k):
    return "".join(f"{key},{m}|{l}|{r}\n" for key, e, m, l, r in recs if len(key) == k)


STAGES = ("s4", "s5_sort", "s5_fold", "s6", "s7_sort", "s7_fold", "s8")


def run_stages(rows, p):
    """every stage's record set, by name (bubble == 0: steps 5-7 are skipped and absent)"""
    st = {"s4": binarize(rows, p)}
    cur = st["s4"]
    if p["bubble"]:
        st["s5_sort"] = sort_records(cur)
        st["s5_fold"] = fork_filter(st["s5_sort"], False, p)
        st["s6"] = reflect(st["s5_fold"])
        st["s7_sort"] = sort_records(st["s6"])
        st["s7_fold"] = cur = fork_filter(st["s7_sort"], True, p)
    st["s8"] = full_kmers(cur)
    return st


def run_text(rows, p):
    return to_text(run_stages(rows, p)["s8"], p["k"])


def handover(text):
    """what rfx_dyn_binarize form 0 makes of the stage's text"""
    out = []
    for row in text.splitlines():
        kmer, attr = row.split(",")
        m, l, r = (int(x) for x in attr.split("|"))
        out.append((kmer[:-1], kmer[-1], 1, l, r))
    return out


def load_case(z, name):
    """a case of tests/golden/ksort_vectors.npz -> (params, rows, {stage: records}, text)"""
    v = z[name + "/params"]
    p = dict(k=int(v[0]), max_k=int(v[1]), min_error_cov=int(v[2]), max_cov=int(v[3]), bubble=int(v[4]),
             min_repeat_fold=float(z[name + "/fold"][0]))

    def strings(key):
        b, off = z[key].tobytes().decode(), z[key + "_off"]
        return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    src = str(z[name + "/seqs_from"]) if name + "/seqs_from" in z.files else name
    st, prev = {}, None
    for s in STAGES:
        if f"{name}/{s}_mlr" not in z.files:
            continue
        mlr = z[f"{name}/{s}_mlr"]
        if s == "s8" and f"{src}/s8_key" not in z.files:
            seqs = [(ln.split(",")[0], "") for ln in z[name + "/text"].tobytes().decode().splitlines()]
        elif f"{src}/{s}_perm" in z.files:
            seqs = [prev[i] for i in z[f"{src}/{s}_perm"]]
        else:
            seqs = list(zip(strings(f"{src}/{s}_key"), strings(f"{src}/{s}_ext")))
        prev = seqs
        st[s] = [(a, b, int(m), int(l), int(r)) for (a, b), (m, l, r) in zip(seqs, mlr)]
    return p, strings(src + "/rows"), st, z[name + "/text"].tobytes().decode()
