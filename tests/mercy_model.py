"""The mercy k-mer stage (Count_<k>_mercy) as string slicing: what P/ReflexivDSDynamicMercyKmer.java
`assemblyFromKmer` (:157-322) computes, written from the rules of section 28 and sharing no code with the library.  The vectors of
tests/golden/mercy_vectors.npz (made by the reference's own classes) decide; tests/test_mercy_model.py holds this model to them."""

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
INDEX_LIMIT = 30000        # the reference stores indices clamped here: longer reads are refused by the library


def letters(s):
    """any base other than A, C, G reads as T (lower case too)"""
    return "".join(c if c in "ACG" else "T" for c in s)


def rc(s):
    return "".join(_COMP[c] for c in reversed(s))


def canon(s):
    return min(s, rc(s))


def solid_set(count_rows, k):
    """the k-mers of the `KMER,count` rows whose k-mer has k bases; a leading '(' of the k-mer is dropped, the count is not read"""
    out = set()
    for row in count_rows:
        kmer = row.rstrip("\r\n").split(",", 1)[0]
        if kmer.startswith("("):
            kmer = kmer[1:]
        if len(kmer) == k:
            out.add(letters(kmer))
    return out


def gives_nothing(read, k, front_clip, end_clip):
    n = len(read)
    return (n - k - end_clip + 1 <= 0 or front_clip > n or n - 15 - end_clip <= 1 or
            (n >= 32 and letters(read[:31]) == "A" * 31))


def hits(read, k, front_clip, end_clip, solid):
    """the window positions whose canonical k-mer is solid, absolute in the read"""
    if gives_nothing(read, k, front_clip, end_clip):
        return []
    s = letters(read)
    return [p for p in range(front_clip, len(s) - end_clip - k + 1) if canon(s[p:p + k]) in solid]


def kept_ranges(hit_list, k):
    """(a, b) for neighbouring hits a < b whose gap g = b - a - 1 is kept: g >= 1 and not k - 1 <= g <= k + 1"""
    out = []
    for a, b in zip(hit_list, hit_list[1:]):
        g = b - a - 1
        if g >= 1 and not (k - 1 <= g <= k + 1):
            out.append((a, b))
    return out


def mercy_kmers(reads, k, front_clip, end_clip, solid):
    """the mercy k-mers in output order (read, position); duplicates are not merged"""
    out = []
    for read in reads:
        s = letters(read)
        for a, b in kept_ranges(hits(read, k, front_clip, end_clip, solid), k):
            out += [canon(s[j:j + k]) for j in range(a + 1, b)]
    return out


def mercy_text(count_rows, reads, k, front_clip=0, end_clip=0):
    return "".join(f"{m},1\n" for m in mercy_kmers(reads, k, front_clip, end_clip, solid_set(count_rows, k)))


def key_of(kmer):
    """a k-mer as the counter's key: 2 bits a base, the last base in the lowest bits"""
    v = 0
    for c in kmer:
        v = (v << 2) | "ACGT".index(c)
    return v
