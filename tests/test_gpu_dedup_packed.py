"""The contig de-duplication on the PACKED contig set that stays in HBM (rfx_dev_contigs_*, rfx_dev_dedup_contigs; DESIGN.md section
16): pack / unpack / from-text / to-text against a numpy statement of the layout (raw words, zero padding bits, offsets, lengths)
and a Python statement of the text, every shift of the word-wise merge against the oracle, the reference-made vectors and the
random sets of tests/test_gpu_dedup.py through both resident routes, the capacity / argument contracts, and all of it again with
every allocation poisoned.  The checkers are the existing ones: tests/golden/dedup_vectors.npz and oracle.dedup_contigs."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_oracle_dedup import VEC, cases, unpack

pytestmark = pytest.mark.gpu

OK, E_ARG, E_CAP = 0, -1, -2
FILL = 0xA5
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 299, 300, 310, 311, 1000)
LINE = 10_000_000
COMP = str.maketrans("ACGT", "TGCA")


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


def rc(s):
    return s.translate(COMP)[::-1]


def rand_seq(rng, n):
    return "".join("ACGT"[b] for b in rng.integers(0, 4, n))


# ---- a numpy statement of the layout and a Python statement of the text --------------------------------------------------------------
CODE = np.full(256, 3, np.uint64)
CODE[ord("A")], CODE[ord("C")], CODE[ord("G")] = 0, 1, 2


def words_of(s):
    """letters -> 64-bit words, 32 bases each, the first in the two highest bits, 0 behind the last base; A0 C1 G2, anything else 3"""
    codes = CODE[np.frombuffer(s.encode(), np.uint8)]
    nw = (len(codes) + 31) // 32
    c = np.zeros(nw * 32, np.uint64)
    c[:len(codes)] = codes
    return np.bitwise_or.reduce(c.reshape(nw, 32) << (np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)), axis=1) if nw else np.zeros(0, np.uint64)


def raw_equals(pk, contigs, tag):
    """the arrays in HBM are the numpy packer's of `contigs`: words (so every padding bit is 0), word offsets, lengths"""
    words, word_off, length = pk.host()
    ww = [words_of(s) for s in contigs]
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in ww])]).astype(np.int64)
    assert pk.n == len(contigs), (tag, pk.n, len(contigs))
    assert np.array_equal(length, np.array([len(s) for s in contigs], np.int64)), (tag, "len")
    assert np.array_equal(word_off, want_off), (tag, "word_off")
    want = np.concatenate(ww) if ww else np.zeros(0, np.uint64)
    assert words.shape == want.shape and np.array_equal(words, want), (tag, "words")


def as_t(s):
    """what a packed contig reads back as: every letter that is not ACG is T"""
    return "".join(ch if ch in "ACG" else "T" for ch in s)


def text_of(contigs, min_contig):
    """TagRowContigDSID + changeLine: the contigs of at least min_contig bases, idx = the position among all"""
    out = []
    for i, s in enumerate(contigs):
        if len(s) < min_contig:
            continue
        out.append(f">Contig-{len(s)}-{i}\n" + "\n".join(s[j:j + LINE] for j in range(0, len(s), LINE)) + "\n")
    return "".join(out)


def path_text(contigs, eol="\n", junk=True):
    """the contig text the path writes: headers and the sequence at 100 columns (a junk line ahead of the first header)"""
    out = ["not a header" + eol + eol] if junk else []
    for i, s in enumerate(contigs):
        out.append(f">Contig-{len(s)}-{i}" + eol + "".join(s[j:j + 100] + eol for j in range(0, len(s), 100)))
    return "".join(out)


def on_device(text):
    import torch
    t = torch.from_numpy(np.frombuffer(text.encode(), np.uint8).copy()).cuda() if text else torch.zeros(1, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t, len(text)


def device_text(rfx, pk, min_contig):
    d_text, ln, nc = rfx.contigs_to_text_dev(pk, min_contig)
    return bytes(d_text[:ln].cpu().numpy()).decode(), nc


# ---- 1. pack / unpack / from-text / to-text --------------------------------------------------------------------------------------------
def mixed_contigs(rng, n):
    """n contigs whose lengths cycle through LENGTHS, letters ACGT with N and lower case among them"""
    alphabet = np.frombuffer(b"ACGTACGTACGTNacgtn", np.uint8)
    return [alphabet[rng.integers(0, len(alphabet), LENGTHS[i % len(LENGTHS)])].tobytes().decode() for i in range(n)]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_pack_unpack_and_the_two_texts_against_numpy(rfx, n):
    """contigs of 0..1000 bases around every word edge, N and lower case included (code 3): the words, offsets and lengths in HBM
    are the numpy packer's, unpack(pack(x)) = x with every non-ACGT letter read as T, the path's text (100 columns, "\\n" and
    "\\r\\n", a junk line ahead, empty contigs) gives the same set, and to-text is the Python statement of the format"""
    contigs = mixed_contigs(np.random.default_rng(90 + n), n)
    if n >= 255:
        assert {len(s) for s in contigs} == set(LENGTHS) and any("N" in s for s in contigs) and any("a" in s for s in contigs)
    pk = rfx.contigs_pack(contigs)
    raw_equals(pk, contigs, ("pack", n))
    assert rfx.contigs_unpack(pk) == [as_t(s) for s in contigs]
    for eol in ("\n", "\r\n"):
        d_text, ln = on_device(path_text(contigs, eol))
        ft = rfx.contigs_from_text_dev(d_text, ln)
        raw_equals(ft, contigs, ("from_text", n, eol))
    for min_contig in (0, 32, 500):
        text, nc = device_text(rfx, pk, min_contig)
        assert text == text_of([as_t(s) for s in contigs], min_contig), (n, min_contig)
        assert nc == sum(1 for s in contigs if len(s) >= min_contig)


def test_from_text_takes_any_line_width_and_a_text_without_a_last_line_end(rfx):
    contigs = mixed_contigs(np.random.default_rng(96), 40)
    text = "".join(f">c{i}\n" + "\n".join(s[j:j + w] for j in range(0, len(s), w)) + "\n" for i, (s, w) in enumerate(zip(contigs, itertools.cycle((1, 7, 33, 2000)))))
    for t in (text, text.rstrip("\n"), ">only a header", "no header at all\nACGT\n"):
        d_text, ln = on_device(t)
        want = contigs if t.startswith(">c0") else [""] if t.startswith(">") else []
        raw_equals(rfx.contigs_from_text_dev(d_text, ln), want, ("widths", t[:12]))


def test_to_text_breaks_a_line_after_ten_million_bases(rfx):
    """one contig of 10,000,000 bases (one full line, no break), one of 10,000,001 (a second line of one base) and a short one
    behind them: the line break and the idx; and the text read back (lines of 10,000,000 columns) gives the same words"""
    rng = np.random.default_rng(97)
    nuc = np.frombuffer(b"ACGT", np.uint8)
    contigs = [nuc[rng.integers(0, 4, L)].tobytes().decode() for L in (LINE, 40, LINE + 1, 600)]
    pk = rfx.contigs_pack(contigs)
    d_text, ln, nc = rfx.contigs_to_text_dev(pk, 500)
    got = bytes(d_text[:ln].cpu().numpy()).decode()
    want = text_of(contigs, 500)
    assert nc == 3 and len(got) == len(want) and got == want
    assert want.count("\n") == 2 + 3 + 2                # (header + lines: one, two, one)
    back = rfx.contigs_from_text_dev(d_text, ln)
    words, word_off, length = back.host()
    assert list(length) == [LINE, LINE + 1, 600]
    assert np.array_equal(words, np.concatenate([words_of(contigs[i]) for i in (0, 2, 3)]))


# ---- 2. every shift of the word-wise merge ---------------------------------------------------------------------------------------------
def shift_set(strand, side, Ls):
    """66 pairs [S, short]: S of Ls + f bases and a short contig that overlaps one of its ends by 500 bases and brings a new flank
    of f = 0..65 bases (left: flank + S[:500], right: S[L-500:] + flank), as is or reverse-complemented -> (contigs, the 66 merged
    contigs flank + S resp. S + flank)"""
    rng = np.random.default_rng(7)
    contigs, merged = [], []
    for f in range(66):
        L = Ls + f
        S, flank = rand_seq(rng, L), rand_seq(rng, f)
        short = flank + S[:500] if side == "left" else S[L - 500:] + flank
        merged.append(flank + S if side == "left" else S + flank)
        contigs += [S, rc(short) if strand == "rc" else short]
    return contigs, merged


def grow_twice_set(strand):
    """40 triples [s1, S, s2]: S of 1500 + f bases, s1 = a left flank of f + 1 bases on S[:500], s2 = S[L-450:] with a right flank of
    37 - f % 37 + 1 bases -> (contigs, the 40 contigs a + S + b): the long contig grows twice, through both work buffers"""
    rng = np.random.default_rng(11)
    contigs, merged = [], []
    for f in range(40):
        L = 1500 + f
        S, a, b = rand_seq(rng, L), rand_seq(rng, f + 1), rand_seq(rng, 37 - f % 37 + 1)
        s1, s2 = a + S[:500], S[L - 450:] + b
        if strand == "rc":
            s1, s2 = rc(s1), rc(s2)
        contigs += [s1, S, s2]
        merged.append(a + S + b)
    return contigs, merged


def merges_equal_the_oracle(rfx, contigs, merged, tag):
    """asserted on the ORACLE's output first: every one of the merged contigs (or its reverse complement) is among the round-3
    contigs; then dedup_dev on the packed set gives the oracle's contigs, rounds and text exactly, in words that keep the invariant"""
    want = O.dedup_contigs(contigs)
    final = set(want["rounds"][2])
    assert sum(1 for m in merged if m in final or rc(m) in final) == len(merged) == len(final), tag
    pk = rfx.contigs_pack(contigs)
    out, rn = rfx.dedup_dev(pk)
    assert rn == [len(r) for r in want["rounds"]], tag
    got = rfx.contigs_unpack(out)
    assert got == want["rounds"][2], (tag, [len(x) for x in got], [len(x) for x in want["rounds"][2]])
    raw_equals(out, got, (tag, "invariant"))
    assert device_text(rfx, out, 500)[0] == want["text"], tag


@pytest.mark.parametrize("strand,side,Ls", list(itertools.product(("fwd", "rc"), ("left", "right"), (700, 2100, 4100))))
def test_every_shift_of_the_word_wise_merge(rfx, strand, side, Ls):
    """flanks of 0..65 bases ahead of and behind long contigs of Ls + f bases (every shift of either piece against the output words,
    twice over), the short contig on either strand (forward: merged in round 2, reverse complement: in round 1), the three
    probe-window regimes (under 2000, under 4000, from 4000 on)"""
    contigs, merged = shift_set(strand, side, Ls)
    assert len(merged) == 66
    merges_equal_the_oracle(rfx, contigs, merged, (strand, side, Ls))


@pytest.mark.parametrize("strand", ["fwd", "rc"])
def test_a_long_contig_that_grows_twice(rfx, strand):
    contigs, merged = grow_twice_set(strand)
    assert len(merged) == 40
    merges_equal_the_oracle(rfx, contigs, merged, ("twice", strand))


# ---- 3. the reference-made sets and the larger random sets, through both resident routes -----------------------------------------------
def both_routes(rfx, contigs, min_contig, want_final, want_text, want_rounds, tag):
    pk = rfx.contigs_pack(contigs)
    out, rn = rfx.dedup_dev(pk)
    assert rn == want_rounds, tag
    got = rfx.contigs_unpack(out)
    assert got == want_final, (tag, "pack route", [len(x) for x in got], [len(x) for x in want_final])
    raw_equals(out, got, (tag, "invariant"))
    d_text, ln = on_device(path_text(contigs, junk=False))
    ft = rfx.contigs_from_text_dev(d_text, ln)
    out2, rn2 = rfx.dedup_dev(ft)
    assert rn2 == want_rounds, tag
    assert device_text(rfx, out2, min_contig) == (want_text, sum(1 for s in want_final if len(s) >= min_contig)), (tag, "text route")
    w1, w2 = out.host(), out2.host()
    assert all(np.array_equal(a, b) for a, b in zip(w1, w2)), (tag, "the two routes")


@pytest.mark.parametrize("case", cases())
def test_packed_dedup_equals_the_reference_classes(rfx, case):
    z = np.load(VEC)
    contigs = unpack(z, case + "/in")
    both_routes(rfx, contigs, 500, unpack(z, f"{case}/round3"), bytes(z[case + "/text"]).decode(),
                [len(unpack(z, f"{case}/round{r}")) for r in (1, 2, 3)], case)


def larger_set(seed):
    """the random sets of tests/test_gpu_dedup.py: both strands, RC pieces with new flanks, forward pieces, near-copies, repeats
    shared between contigs, long contigs"""
    rng = np.random.default_rng(seed)
    base = []
    rep = rand_seq(rng, 400)
    for L in list(rng.integers(300, 9000, 30)) + [120_000, 65_000, 31 * 200, 31 * 97 + 30]:
        s = rand_seq(rng, int(L))
        if rng.random() < 0.3 and L > 1500:
            p = int(rng.integers(100, L - 500))
            s = s[:p] + rep + s[p + 400:]
        base.append(s)
        r = rng.random()
        if r < 0.55:
            base.append(rc(s))
        elif r < 0.7:
            a, b = int(rng.integers(0, 200)), int(rng.integers(0, 200))
            base.append(rc(rand_seq(rng, a) + s[int(L) // 5: int(L) * 4 // 5] + rand_seq(rng, b)))
        elif r < 0.8:
            base.append(s[int(L) // 10: int(L) // 2])
        elif r < 0.9:
            t = list(rc(s))
            for p in rng.integers(0, len(t), max(1, len(t) // 300)):
                t[p] = "ACGT"[("ACGT".index(t[p]) + 1) % 4]
            base.append("".join(t))
    base += [rand_seq(rng, int(L)) for L in rng.integers(50, 400, 8)]
    order = rng.permutation(len(base))
    return [base[i] for i in order]


@functools.lru_cache(maxsize=None)
def larger_set_and_oracle(seed):
    contigs = larger_set(seed)
    return contigs, O.dedup_contigs(contigs)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_packed_dedup_equals_the_oracle_on_larger_sets(rfx, seed):
    contigs, want = larger_set_and_oracle(seed)
    both_routes(rfx, contigs, 500, want["rounds"][2], want["text"], [len(r) for r in want["rounds"]], seed)


# ---- 4. contracts ------------------------------------------------------------------------------------------------------------------------
def sentinel(cap_n, cap_words):
    """an output set whose every tensor is filled with 0xA5"""
    import torch
    from reflexiv_amd.api import ContigsPacked
    d = ContigsPacked(cap_n, cap_words)
    for t in d.tensors():
        t.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    return d


def untouched(d):
    import torch
    return all(bool((t.view(torch.uint8) == FILL).all()) for t in d.tensors())


def small_set():
    rng = np.random.default_rng(98)
    seqs = [rand_seq(rng, L) for L in (900, 1500, 700, 2500, 640, 45)]
    return [seqs[0], rc(seqs[1]), seqs[2], seqs[1], seqs[3], rc(seqs[0]), seqs[4], seqs[5]]


def test_a_short_output_is_refused_with_the_needs_and_nothing_written(rfx):
    """pack, from-text and dedup with cap_n = need - 1, then cap_words = need - 1: RFX_E_CAP with need_n / need_words set and every
    output tensor (0xA5) as it was; with exactly the needs the same call succeeds"""
    L, ctx = rfx.L, rfx.ctx
    contigs = small_set()
    pk = rfx.contigs_pack(contigs)
    ci = pk._c()
    off = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)
    bases = np.frombuffer("".join(contigs).encode(), np.uint8).copy()
    d_text, ln = on_device(path_text(contigs))
    rn = (C.c_int64 * 3)()
    ops = {
        "rfx_dev_contigs_pack": lambda co: L.rfx_dev_contigs_pack(ctx, bases.ctypes.data, off.ctypes.data, len(contigs), C.byref(co)),
        "rfx_dev_contigs_from_text": lambda co: L.rfx_dev_contigs_from_text(ctx, d_text.data_ptr(), ln, C.byref(co)),
        "rfx_dev_dedup_contigs": lambda co: L.rfx_dev_dedup_contigs(ctx, C.byref(ci), C.byref(co), C.addressof(rn)),
    }
    for name, call in ops.items():
        big = sentinel(pk.n + 4, pk.words + 8)
        co = big._c()
        assert call(co) == OK, name
        need_n, need_w = int(co.need_n), int(co.need_words)
        assert int(co.n) == need_n and 0 < need_n <= pk.n and 0 < need_w <= pk.words, (name, need_n, need_w)
        exact = sentinel(need_n, need_w)
        assert call(exact._c()) == OK and not untouched(exact), name
        for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
            d = sentinel(cap_n, cap_w)
            co = d._c()
            co.need_n = co.need_words = -77
            assert call(co) == E_CAP, (name, cap_n, cap_w)
            assert (int(co.need_n), int(co.need_words)) == (need_n, need_w), name
            assert untouched(d), (name, cap_n, cap_w)
    # dedup: no marker row is left over here, so the input's sizes suffice (the bound of include/reflexiv_hip.h)
    assert need_n < pk.n and need_w <= pk.words
    # unpack with a capacity one short: RFX_E_CAP, *out_n set, nothing written
    surv = rfx.contigs_unpack(pk)
    nb = sum(map(len, surv))
    for cap_b, cap_c in ((nb - 1, pk.n), (nb, pk.n - 1), (nb, pk.n)):
        ob, oo, m = np.full(nb + 8, FILL, np.uint8), np.full(pk.n + 9, -77, np.int64), C.c_int64(-77)
        st = L.rfx_dev_contigs_unpack(ctx, C.byref(ci), ob.ctypes.data, cap_b, oo.ctypes.data, cap_c, C.addressof(m))
        assert m.value == pk.n
        if (cap_b, cap_c) == (nb, pk.n):
            assert st == OK and ob[:nb].tobytes().decode() == "".join(surv) and (ob[nb:] == FILL).all() and (oo[pk.n + 1:] == -77).all()
        else:
            assert st == E_CAP and (ob == FILL).all() and (oo == -77).all()


def test_a_text_buffer_one_byte_short(rfx):
    """rfx_dev_contigs_to_text with cap = length - 1: RFX_E_CAP, the needed length, nothing at or past cap written"""
    import torch
    contigs = small_set()
    pk = rfx.contigs_pack(contigs)
    want = text_of(contigs, 500)
    need = len(want)
    for cap in (need - 1, need // 2, 0, need):
        d_text = torch.full((need + 16,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ln, nc = C.c_int64(-77), C.c_int64(-77)
        st = rfx.L.rfx_dev_contigs_to_text(rfx.ctx, C.byref(pk._c()), 500, d_text.data_ptr(), cap, C.addressof(ln), C.addressof(nc))
        assert (st, ln.value, nc.value) == (OK if cap >= need else E_CAP, need, 7), cap
        assert bool((d_text[cap:] == FILL).all()) and bytes(d_text[:cap].cpu().numpy()).decode() == want[:cap], cap


def test_an_empty_set_through_every_entry_point(rfx):
    pk = rfx.contigs_pack([])
    assert pk.n == 0 and pk.words == 0 and rfx.contigs_unpack(pk) == []
    out, rn = rfx.dedup_dev(pk)
    assert out.n == 0 and rn == [0, 0, 0] and int(out.word_off[0]) == 0
    assert device_text(rfx, out, 0) == ("", 0)
    for text in ("", "\n\r\n", "ACGT\n"):
        d_text, ln = on_device(text)
        ft = rfx.contigs_from_text_dev(d_text, ln)
        assert ft.n == 0 and int(ft.word_off[0]) == 0
    # contigs of no bases are contigs: they keep their positions
    pk = rfx.contigs_pack(["", "", ""])
    raw_equals(pk, ["", "", ""], "empty contigs")
    out, rn = rfx.dedup_dev(pk)
    assert rn == [3, 3, 3] and rfx.contigs_unpack(out) == ["", "", ""]
    assert device_text(rfx, out, 0)[0] == ">Contig-0-0\n\n>Contig-0-1\n\n>Contig-0-2\n\n"
    assert rfx.dedup_contigs([], 100) == ([], "", [0, 0, 0])


def test_null_pointers_and_negative_counts_are_refused(rfx):
    L, ctx = rfx.L, rfx.ctx
    contigs = small_set()
    pk = rfx.contigs_pack(contigs)
    ci = pk._c()
    d = sentinel(pk.n, pk.words)
    off = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)
    bases = np.frombuffer("".join(contigs).encode(), np.uint8).copy()
    d_text, ln = on_device(path_text(contigs))
    m, tl = C.c_int64(-77), C.c_int64(-77)
    ob, oo = np.full(64, FILL, np.uint8), np.full(16, -77, np.int64)

    def holed(which):
        co = d._c()
        setattr(co, which, None)
        return co
    neg = pk._c()
    neg.n = -1
    calls = [
        L.rfx_dev_contigs_pack(None, bases.ctypes.data, off.ctypes.data, len(contigs), C.byref(d._c())),
        L.rfx_dev_contigs_pack(ctx, None, off.ctypes.data, len(contigs), C.byref(d._c())),
        L.rfx_dev_contigs_pack(ctx, bases.ctypes.data, None, len(contigs), C.byref(d._c())),
        L.rfx_dev_contigs_pack(ctx, bases.ctypes.data, off.ctypes.data, -1, C.byref(d._c())),
        L.rfx_dev_contigs_pack(ctx, bases.ctypes.data, off.ctypes.data, len(contigs), None),
        L.rfx_dev_contigs_from_text(ctx, None, ln, C.byref(d._c())),
        L.rfx_dev_contigs_from_text(ctx, d_text.data_ptr(), -1, C.byref(d._c())),
        L.rfx_dev_contigs_from_text(ctx, d_text.data_ptr(), ln, None),
        L.rfx_dev_dedup_contigs(ctx, None, C.byref(d._c()), None),
        L.rfx_dev_dedup_contigs(ctx, C.byref(ci), None, None),
        L.rfx_dev_dedup_contigs(ctx, C.byref(neg), C.byref(d._c()), None),
        L.rfx_dev_contigs_unpack(ctx, None, ob.ctypes.data, 64, oo.ctypes.data, 15, C.addressof(m)),
        L.rfx_dev_contigs_unpack(ctx, C.byref(ci), ob.ctypes.data, 64, None, 15, C.addressof(m)),
        L.rfx_dev_contigs_unpack(ctx, C.byref(ci), ob.ctypes.data, 64, oo.ctypes.data, 15, None),
        L.rfx_dev_contigs_unpack(ctx, C.byref(ci), ob.ctypes.data, -1, oo.ctypes.data, 15, C.addressof(m)),
        L.rfx_dev_contigs_to_text(ctx, None, 500, d_text.data_ptr(), 16, C.addressof(tl), None),
        L.rfx_dev_contigs_to_text(ctx, C.byref(ci), 500, None, 16, C.addressof(tl), None),
        L.rfx_dev_contigs_to_text(ctx, C.byref(ci), 500, d_text.data_ptr(), 16, None, None),
        L.rfx_dev_contigs_to_text(ctx, C.byref(ci), 500, d_text.data_ptr(), -1, C.addressof(tl), None),
    ]
    for which in ("words", "word_off", "len"):
        calls.append(L.rfx_dev_dedup_contigs(ctx, C.byref(holed(which)), C.byref(d._c()), None))
        calls.append(L.rfx_dev_dedup_contigs(ctx, C.byref(ci), C.byref(holed(which)), None))
        calls.append(L.rfx_dev_contigs_pack(ctx, bases.ctypes.data, off.ctypes.data, len(contigs), C.byref(holed(which))))
    assert calls == [E_ARG] * len(calls), calls
    assert untouched(d) and m.value == -77 and tl.value == -77 and (ob == FILL).all() and (oo == -77).all()
    # an input whose offsets and lengths disagree is refused before any kernel reads it
    import torch
    bad = rfx.contigs_pack(contigs)
    bad.len[2] += 40
    torch.cuda.synchronize()
    assert L.rfx_dev_dedup_contigs(ctx, C.byref(bad._c()), C.byref(d._c()), None) == E_ARG and untouched(d)


# ---- 5. poisoned allocations ---------------------------------------------------------------------------------------------------------------
def test_packed_dedup_holds_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it, so a producer that
    relied on zeroed memory for its padding bits fails the raw-word checks above.  A child process: the mask is read once per
    process."""
    import subprocess
    import sys
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
