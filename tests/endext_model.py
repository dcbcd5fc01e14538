"""String model of the end extension of contigs from alignment rows (Assembly_intermediate/07EndExtend):
P/ReflexivDSDynamicKmerMapping.java behind its aligner -- SAMString2ROW (:369-388), DSProcessSAMandExtendContigs (:564-994), the union
with 05FixingAgain and the sort by ID (:320-331), DSExtendContigs (:413-562) and TagStringContigRDDID (:1268-1286).  Test
infrastructure, imported by the tests and by tests/golden/make_endext_vectors.py only.

A contig is (ID, bases) as a row of 05FixingAgain holds it, ID = Contig_<L>_<left>_<right>_<idx>.  An alignment row is (name, start,
cigar, seq), name = ID, ID-L or ID-R.  All alignment rows form ONE logical partition (the stated deviation): every row of a contig is
counted, whatever the order of the rows.  Where the reference would throw -- a CIGAR that is not ([0-9]+[A-Z=])+, a start that is no
int, an overhang that indexes outside seq, each on a row that is no repeat marker -- the model raises ValueError (RFX_E_ARG)."""
import re

LONGEST = 300                                                      # longestExtend (:567)
NEAR = 10                                                          # `refStart >= 10` / `refTailLength >= 10` skip a row
END = 200                                                          # refLength of a -R row (:751)
CIGAR = re.compile(r"(?:[0-9]+[A-Z=])+")
ID = re.compile(r"Contig_(0|[1-9][0-9]*)_(0|-?[1-9][0-9]*)_(0|-?[1-9][0-9]*)_(0|[1-9][0-9]*)")
LETTERS = "ACGT"


def split_rows(lines):
    """SAMString2ROW (:369-388): split("\\t") drops trailing empty fields; fewer than 4 fields skip the line"""
    out = []
    for line in lines:
        f = line.rstrip("\r\n").split("\t")
        while f and f[-1] == "":
            f.pop()
        if len(f) >= 4:
            out.append((f[0], f[1], f[2], f[3]))
    return out


def sam_to_rows(lines):
    """full SAM lines -> the four-column rows, as the commented awk of :1189: header and `*` lines skipped, fields 3, 4, 6 and 10"""
    out = []
    for line in lines:
        f = line.rstrip("\n").split("\t")
        if line.startswith("@") or len(f) < 11 or f[2] == "*":
            continue
        out.append("\t".join((f[2], f[3], f[5], f[9])))
    return out


def char2int(c):
    return {"a": 0, "A": 0, "c": 1, "C": 1, "g": 2, "G": 2}.get(c, 3)


def name_parts(name):
    """-> (ID, side): side 'L', 'R' or '' (one suffix is stripped)"""
    if name.endswith("-L") or name.endswith("-R"):
        return name[:-2], name[-1]
    return name, ""


def is_marker(side, seq):
    """-> (left repeat, right repeat); the marker test comes before any CIGAR parsing"""
    if side == "L":
        return (seq == "L", False)
    if side == "R":
        return (False, seq == "R")
    return (seq in ("L", "L-R"), seq in ("R", "L-R"))


def parse_int(s):
    if not re.fullmatch(r"[+-]?[0-9]{1,10}", s) or not -(1 << 31) <= int(s) < (1 << 31):
        raise ValueError(f"start {s!r} is no int")
    return int(s)


def contributions(name, start, cigar, seq):
    """a row that is no marker -> (the bases it adds to the left table from j = 0, those it adds to the right table), uncut"""
    ident, side = name_parts(name)
    start = parse_int(start)
    if not CIGAR.fullmatch(cigar):
        raise ValueError(f"CIGAR {cigar!r}")
    ops = [(int(n), t) for n, t in re.findall(r"([0-9]+)([A-Z=])", cigar)]
    if any(n >= 10 ** 9 for n, _ in ops):
        raise ValueError(f"CIGAR {cigar!r}: an operation of 10^9 or more")
    left = right = ""
    if side in ("L", "") and ops[0][1] == "S" and start < NEAR:
        o = ops[0][0] - start
        if o > 0:
            if o >= len(seq):
                raise ValueError("left overhang outside seq")
            left = seq[o::-1]                                      # seq[o], seq[o-1], ..., seq[0]: o + 1 bases
    if side in ("R", "") and ops[-1][1] == "S":
        first_m = next((i for i, (_, t) in enumerate(ops) if t == "M"), 0)
        align = sum(-n if t == "I" else n for n, t in ops[first_m:len(ops) - 1])
        ref = END if side == "R" else int(ident.split("_")[1])
        tail = ref - (align + start - 1)
        if tail < NEAR:
            o = ops[-1][0] - tail
            if o > 0:
                if o > len(seq):
                    raise ValueError("right overhang outside seq")
                right = seq[len(seq) - o:]
    return left, right


class Pile:
    def __init__(self):
        self.tab = [[[0] * 4 for _ in range(LONGEST)] for _ in range(2)]
        self.rep = [0, 0]
        self.longest = [0, 0]                                      # uncut, for the generator's facts
        self.tie = False

    def add(self, name, start, cigar, seq):
        side = name_parts(name)[1]
        ml, mr = is_marker(side, seq)
        if ml or mr:
            self.rep[0] += ml
            self.rep[1] += mr
            return
        for s, bases in enumerate(contributions(name, start, cigar, seq)):
            self.longest[s] = max(self.longest[s], len(bases))
            for j, c in enumerate(bases[:LONGEST]):
                self.tab[s][j][char2int(c)] += 1

    def consensus(self, s):
        out = []
        for row in self.tab[s]:
            hi = max(row)
            if hi:
                self.tie |= row.count(hi) > 1
                out.append(LETTERS[max(c for c in range(4) if row[c] == hi)])      # a tie goes to the HIGHER code
        return "".join(out)


def piles(rows):
    """{ID: Pile} over every row, whatever the order"""
    out = {}
    for name, start, cigar, seq in rows:
        out.setdefault(name_parts(name)[0], Pile()).add(name, start, cigar, seq)
    return out


def consensus_rows(rows, facts=None):
    """DSProcessSAMandExtendContigs over the rows sorted by name in ONE partition -> [(ID, "L-" + ...), (ID, "R-" + ...)] per ID in
    byte order.  No rows at all: the reference's ("first", "L-"), ("first", "R-")"""
    ps = piles(rows)
    out = []
    for ident in sorted(ps):
        p = ps[ident]
        lc, rc = p.consensus(0), p.consensus(1)
        out.append((ident, "L-" + ("l1-" if p.rep[0] >= 2 else "") + lc))
        out.append((ident, "R-" + ("r1-" if p.rep[1] >= 2 else "") + rc))
        if facts is not None:
            facts["tie"] = facts.get("tie", False) or p.tie
            facts["cut"] = facts.get("cut", False) or max(p.longest) > LONGEST
    if not ps:
        out = [("first", "L-"), ("first", "R-")]
    return out


def extend(contigs, cons):
    """the union sorted by ID (stable, byte order) + DSExtendContigs -> ["<ID>_<ll>_<rl>,<sequence>"] in that order"""
    by = {}
    for ident, s in cons:
        by.setdefault(ident, ["", ""])[0 if s.startswith("L-") else 1] = s[2:]
    out = []
    for ident, bases in sorted(contigs, key=lambda c: c[0]):
        if len(bases) <= 1:
            continue
        lc, rc = by.get(ident, ("", ""))
        f = ident.split("_")
        if re.search(r"l(\d+)-", lc) and int(f[2]) <= 1:          # <= 0 becomes 1; > 0 only where 1 >= the field
            f[2] = "1"
        if re.search(r"r(\d+)-", rc) and int(f[3]) <= 1:
            f[3] = "1"
        out.append("_".join(f) + f"_{len(lc)}_{len(rc)}," + lc[::-1] + bases + rc)
    return out


def tag(strings, max_k):
    """zipWithIndex + TagStringContigRDDID (:1268-1286): the rows of 07EndExtend"""
    out = []
    for i, s in enumerate(strings):
        ident, seq = s.split(",")[:2]
        if len(seq) >= 2 * max_k:
            out.append(f">{ident}_{i},{seq}\n")
    return "".join(out)


def contigs_of_text(text):
    """the rows of 05FixingAgain -> [(ID, bases)]"""
    return [tuple(r.split(",")[:2]) for r in text.splitlines()]


def run_text(contig_text, row_lines, max_k):
    return tag(extend(contigs_of_text(contig_text), consensus_rows(split_rows(row_lines))), max_k)


# ---- what the device computes, per contig of the INPUT set ---------------------------------------------------------------------------
def device_consensus(contigs, row_lines):
    """-> per contig (left consensus from j = 0, right consensus, flags: 1 = left repeat, 2 = right repeat).  A row whose name does
    not match the contig at its <idx> in L, left and right is ignored, before anything of it is looked at"""
    ids = [c[0] for c in contigs]
    for i, ident in enumerate(ids):
        m = ID.fullmatch(ident)
        assert m and int(m.group(4)) == i and int(m.group(1)) == len(contigs[i][1]), ident
    known = set(ids)
    ps = piles([r for r in split_rows(row_lines) if name_parts(r[0])[0] in known])
    out = []
    for ident in ids:
        p = ps.get(ident)
        out.append((p.consensus(0), p.consensus(1), (p.rep[0] >= 2) + 2 * (p.rep[1] >= 2)) if p else ("", "", 0))
    return out


# ---- the order key ---------------------------------------------------------------------------------------------------------------
def order_key(ident):
    """the four decimal fields of an ID as 4-bit characters ordered '-' < '0'..'9' < '_', the end of the text 0: three 64-bit words
    whose order as a 192-bit number is the byte order of the IDs ("Contig_" is common to all).  45 characters at most: L and idx 10
    digits, left and right a sign and 10 digits, three separators"""
    tail = ident[len("Contig_"):]
    assert ID.fullmatch(ident) and len(tail) <= 48, ident
    v = 0
    for c in tail:
        v = (v << 4) | (1 if c == "-" else 12 if c == "_" else 2 + ord(c) - 48)
    v <<= 4 * (48 - len(tail))
    return (v >> 128, (v >> 64) & ((1 << 64) - 1), v & ((1 << 64) - 1))


def device_set(contigs, row_lines, max_k):
    """-> the contigs of 07EndExtend in output order as the device holds them: dicts of bases (reversed left || contig || right, no
    literals), left, right, left_len, right_len (the lengths the ID carries), flags, src_idx and new_idx"""
    cons = device_consensus(contigs, row_lines)
    out, new = [], 0
    for i in sorted(range(len(contigs)), key=lambda j: contigs[j][0]):
        ident, bases = contigs[i]
        if len(bases) <= 1:
            continue
        lc, rc, f = cons[i]
        fl, fr = f & 1, (f >> 1) & 1
        left, right = (int(x) for x in ident.split("_")[2:4])
        rec = dict(bases=lc[::-1] + bases + rc, left=1 if fl and left <= 1 else left, right=1 if fr and right <= 1 else right,
                   left_len=len(lc) + 3 * fl, right_len=len(rc) + 3 * fr, flags=f, src_idx=i, new_idx=new)
        if len(rec["bases"]) + 3 * fl + 3 * fr >= 2 * max_k:
            out.append(rec)
        new += 1
    return out


def set_text(recs):
    """the rows of 07EndExtend out of device_set's records: the literals go back in at the two seams"""
    out = []
    for r in recs:
        fl, fr = r["flags"] & 1, (r["flags"] >> 1) & 1
        cl, cr = r["left_len"] - 3 * fl, r["right_len"] - 3 * fr
        b = r["bases"]
        seq = b[:cl] + "-1l" * fl + b[cl:len(b) - cr] + "r1-" * fr + b[len(b) - cr:]
        out.append(f">Contig_{len(b) - cl - cr}_{r['left']}_{r['right']}_{r['src_idx']}_{r['left_len']}_{r['right_len']}_{r['new_idx']},{seq}\n")
    return "".join(out)


def load_case(z, name):
    """a case of tests/golden/endext_vectors.npz -> (max_k, the contig text, the row lines, the consensus rows, the spliced strings,
    the text of 07EndExtend).  A case named fix_<name> reads the 05FixingAgain text of case <name> of fixing2_vectors.npz"""
    import os
    import numpy as np

    def text(key):
        return z[name + "/" + key].tobytes().decode()

    if name.startswith("fix_"):
        here = os.path.dirname(os.path.abspath(__file__))
        contig_text = np.load(os.path.join(here, "golden", "fixing2_vectors.npz"))[name[4:] + "/text"].tobytes().decode()
    else:
        contig_text = text("contigs")
    cons = [tuple(r.split("\t")) for r in text("cons").splitlines()]
    return int(z[name + "/max_k"][0]), contig_text, text("rows").split("\n")[:-1], cons, text("spliced").splitlines(), text("text")
