"""Brute-force string model of the end mapping (reads onto the contig ends, the front half of the Mapping stage).
The stage's semantics are this project's own -- the reference pipes the reads through an external aligner and a script it does not
ship --, so this model IS the definition the device is held to, byte for byte.  Test infrastructure: plain string slicing for every
target end, read, strand and offset; it shares no code with the library.  (One substring test skips an end whose seed the oriented
read does not contain at all; every offset of the others is tried.)

A contig is (ID, bases) as a row of 05FixingAgain holds it, ID = Contig_<L>_<left>_<right>_<idx>.  A read is a string; every character
other than A, C and G reads as T."""
import numpy as np

END = 200                                                          # bases of a contig end; 2 END bases or more give two targets
LETTERS = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
DEFAULTS = dict(seed=21, min_overlap=31, max_mismatch=2)


def norm(read):
    """the read as its 2-bit codes spell it: A, C, G, anything else T"""
    return "".join(c if c in "ACG" else "T" for c in read)


def revcomp(seq):
    return "".join(COMP[c] for c in reversed(seq))


def ends_of(contigs):
    """-> [(end number, name, target bases, side, whole)] in end order: contig ascending, left (side 0) before right; end number =
    2 contig + side.  whole: the target is the whole contig and has both ends"""
    out = []
    for i, (ident, bases) in enumerate(contigs):
        if len(bases) >= 2 * END:
            out.append((2 * i, ident + "-L", bases[:END], 0, False))
            out.append((2 * i + 1, ident + "-R", bases[len(bases) - END:], 1, False))
        else:
            out.append((2 * i, ident, bases, 0, True))
            out.append((2 * i + 1, ident, bases, 1, True))
    return out


def mismatches(a, b):
    assert len(a) == len(b)
    return sum(x != y for x, y in zip(a, b))


def place(r, T, side, whole, off, seed, min_overlap, max_mismatch):
    """one placement of the oriented read r at offset off of an end of target T -> (v, p, overhang) or None"""
    n = len(r)
    if len(T) < seed:
        return None
    if side == 0:
        if not 1 <= off <= n - seed or r[off:off + seed] != T[:seed]:
            return None
        v = min(n - off, len(T))
        p = n - off - v
        a, b, over = r[off:off + v], T[:v], off
    else:
        if not (0 <= off and off + seed <= n - 1) or r[off:off + seed] != T[len(T) - seed:]:
            return None
        over = n - off - seed
        v = min(off + seed, len(T))
        p = off + seed - v
        a, b = r[p:p + v], T[len(T) - v:]
    if v < min_overlap or mismatches(a, b) > max_mismatch:
        return None
    if whole and p > 0:                                            # bases past both ends of a whole-contig target: neither end emits it
        return None
    return v, p, over


def hits(contigs, reads, seed=21, min_overlap=31, max_mismatch=2):
    """-> [(read, end, strand, offset, v, p, overhang, name, oriented read, target length)] in row order: read, strand, end, offset"""
    ends = ends_of(contigs)
    out = []
    for ri, read in enumerate(reads):
        fw = norm(read)
        for strand, r in enumerate((fw, revcomp(fw))):
            for e, name, T, side, whole in ends:
                if len(T) < seed or (T[:seed] if side == 0 else T[len(T) - seed:]) not in r:
                    continue
                for off in range(len(r)):
                    got = place(r, T, side, whole, off, seed, min_overlap, max_mismatch)
                    if got:
                        out.append((ri, e, strand, off, got[0], got[1], got[2], name, r, len(T)))
    return out


def row_of(hit):
    ri, e, strand, off, v, p, over, name, r, tlen = hit
    if e & 1:
        return f"{name}\t{tlen - v + 1}\t{f'{p}S' if p else ''}{v}M{over}S\t{r}"
    return f"{name}\t1\t{over}S{v}M{f'{p}S' if p else ''}\t{r}"


def rows(contigs, reads, **prm):
    """the row lines (no newline), in row order"""
    return [row_of(h) for h in hits(contigs, reads, **{**DEFAULTS, **prm})]


def fields(hs):
    """the five device arrays of a list of hits"""
    a = np.array([h[:5] for h in hs], np.int32).reshape(-1, 5)
    return {"read": a[:, 0], "end": a[:, 1], "strand": a[:, 2], "offset": a[:, 3], "v": a[:, 4]}


def contig_text(contigs):
    return "".join(f"{i},{b}\n" for i, b in contigs)


def rand_seq(rng, n):
    return "".join(LETTERS[int(x)] for x in rng.integers(0, 4, n))


def planted_case(seed=2026, genome_len=3000, step=3):
    """a random genome, contigs cut from it with gaps of 40 to 120 bases between them, error-free reads of 100 and 150 bases on both
    strands that cover everything -> (genome, [(start, end)] of the contigs, contigs, reads)"""
    rng = np.random.default_rng(seed)
    genome = rand_seq(rng, genome_len)
    spans, pos = [], 150
    for L in (450, 260, 400, 130, 520, 399, 75):
        if pos + L + 150 > genome_len:
            break
        spans.append((pos, pos + L))
        pos += L + int(rng.integers(40, 121))
    contigs = [(f"Contig_{e - s}_{int(rng.integers(-3, 4))}_{int(rng.integers(-3, 4))}_{i}", genome[s:e]) for i, (s, e) in enumerate(spans)]
    reads = []
    for k, start in enumerate(range(0, genome_len - 100 + 1, step)):
        n = 150 if k % 2 and start + 150 <= genome_len else 100
        r = genome[start:start + n]
        reads.append(revcomp(r) if k % 3 == 0 else r)
    return genome, spans, contigs, reads
