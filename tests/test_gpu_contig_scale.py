"""The contig, mapping and mercy stages past the sizes where their launches change shape: 05FixingAgain /
06ContigEnds (rfx_fixing2.hip), 07EndExtend (rfx_endext.hip), 08Extend / 09ExtendAgain (rfx_ctgext.hip), the end mapper
(rfx_endmap.hip) and the mercy stage (rfx_mercy.hip).  Their own files stay inside one look-back scan tile, inside k_sort_small and
inside one trip of the grid-stride loops; here every scanned quantity runs over 4,096 / 4,097 / 8,193 elements with dropped ones in
every tile, the sorts leave k_sort_small for the top-digit path and for two MSD levels, and the read loops of k_mp_scan and k_mc_scan
make a second trip.

Every comparison is exact and against a string model (fixing2_model, endext_model, extend_model, map_model, mercy_model) or a numpy /
dict statement of one that tests/test_contig_scale_inputs.py pins to it on the CPU, where the conditions on the inputs are asserted
too; never against another entry point.  Contig sets are compared through rfx_dev_contigs_unpack and word for word against
words_of_ragged of tests/test_gpu_dynamic_scale.py, record sets with its equals_fast."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import endext_model as E
from tests import extend_model as X
from tests import fixing2_model as F2
from tests import map_model as MP
from tests import mercy_model as MC
from tests import test_gpu_dynamic_scale as S
from tests import test_gpu_endext as TE
from tests import test_gpu_extend as TX
from tests import test_gpu_fixing as TF
from tests import test_gpu_fixing2 as TF2
from tests.test_gpu_dynamic_scale import equals_fast, host_dyn, offsets_of
from tests.test_gpu_fixing import lines
from tests.test_gpu_ksort import upload

pytestmark = pytest.mark.gpu

NUC = np.frombuffer(b"ACGT", np.uint8)
CODE = np.full(256, 3, np.uint8)                                   # any letter other than A, C, G reads as T
CODE[np.frombuffer(b"ACG", np.uint8)] = np.arange(3, dtype=np.uint8)
TILE = 4096                                                        # rfx_scan.hip: LB_TILE
LANE_WINDOW = 64 * TILE                                            # k_scan_lookback: the tiles one lane window covers
SORT_SMALL, SORT_TWO_LEVELS = 2048, 393_216                        # rfx_sort.hip: k_sort_small up to, the top-digit path up to
MARK = np.array([-30000, -7, -1, 0, 1, 2, 9, 12, 123, 30000])      # left / right: every sign and width of the decimal field
MI355X_CUS = 256


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- what the slow string models gave, made once: in this process, or by the parent of the poisoned run ----------------------------------
WANT_ENV = "RFX_CONTIG_SCALE_WANT"                                 # a pickle of {key: value} the parent process wrote
_want = {}


def want(key, make):
    if not _want and os.environ.get(WANT_ENV):
        with open(os.environ[WANT_ENV], "rb") as f:
            _want.update(pickle.load(f))
    if key not in _want:
        _want[key] = make()
    return _want[key]


# ---- strings and words without a loop over the bases ---------------------------------------------------------------------------------------
def strings_of(codes, off):
    return S.strings_of(codes, off)


def codes_of(seqs):
    text = "".join(seqs)
    return CODE[np.frombuffer(text.encode(), np.uint8)] if text else np.zeros(0, np.uint8)


def contig_words_np(seqs):
    """packed_equals' packer (tests/test_gpu_endext.py) without a loop over the contigs: every contig on ceil(len / 32) words, 0 behind
    its last base -> (words, word offsets, lengths)"""
    ln = np.array([len(s) for s in seqs], np.int64)
    off = offsets_of(ln)
    words, woff = S.words_of_ragged(codes_of(seqs), off)
    return words, woff, ln


def packed_equals_fast(rfx, c, seqs, tag):
    """packed_equals of tests/test_gpu_endext.py on the vectorised packer: through rfx_dev_contigs_unpack, and word for word"""
    assert c.n == len(seqs), (tag, c.n, len(seqs))
    got = rfx.contigs_unpack(c)
    if got != list(seqs):
        i = next(j for j, (a, b) in enumerate(zip(got, seqs)) if a != b)
        raise AssertionError((tag, "first contig that differs", i))
    words, woff, ln = c.host()
    w, o, l = contig_words_np(seqs)
    assert np.array_equal(woff, o) and np.array_equal(ln, l), (tag, "offsets / lengths")
    assert np.array_equal(words, w), (tag, "words")


def same_text(got, wanted, tag):
    if got != wanted:
        n = min(len(got), len(wanted))
        i = next((j for j in range(n) if got[j] != wanted[j]), n)
        raise AssertionError((tag, len(got), len(wanted), "first difference at byte", i, got[max(0, i - 60):i + 20], wanted[max(0, i - 60):i + 20]))


def text_from(t, n):
    return bytes(t[:n].cpu().numpy()).decode()


def tiles(flags):
    return [flags[i:i + TILE] for i in range(0, len(flags), TILE)]


def every_tile_has(flags):
    """every FULL tile of 4,096 holds a set flag (the sizes 4,097 and 8,193 end in a tile of one element)"""
    return all(t.any() for t in tiles(np.asarray(flags)) if len(t) == TILE)


# ---- A. 05FixingAgain / 06ContigEnds --------------------------------------------------------------------------------------------------------
FIX2_SIZES = (4096, 4097, 8193, 270_000)
FIX2_MAX_K = 44                                                    # contigs of 62..140 bases: those below 88 are dropped, a third
FIX2_LONG_ONE_IN = 40                                              # a contig of 400..460 bases: the two-record shape of 06ContigEnds
FIX2_CHAIN = (5000, 32, 7)                                         # records, max_k, P of the loop's case


def fix2_records(n):
    """n records in the form of 04Fixing (30-base keys), both markers, contigs of 62..140 bases and one in 40 of 400..460, left / right
    of every sign and width; the last one is kept -> DynRecords"""
    rng = np.random.default_rng(2100 + n)
    L = np.where(rng.random(n) < 1.0 / FIX2_LONG_ONE_IN, rng.integers(400, 461, n), rng.integers(62, 141, n))
    L[n - 1] = max(L[n - 1], 2 * FIX2_MAX_K + 7)                    # the last record is kept: at 4,097 and 8,193 it is a tile of its own
    eo = offsets_of(L - F2.KEY)
    return S.dyn_records(rng.integers(0, 4, F2.KEY * n, dtype=np.uint8), np.arange(n + 1) * F2.KEY, rng.integers(0, 4, eo[-1], dtype=np.uint8), eo,
                         rng.integers(1, 3, n), rng.choice(MARK, n), rng.choice(MARK, n))


def fix2_model(r):
    """the string model on the records of a DynRecords -> (the kept contigs, 05FixingAgain, 06ContigEnds, the text of 09ExtendAgain)"""
    cs = F2.contigs(S.tuples_of(r, "dyn"), F2.default_params(FIX2_MAX_K))
    return cs, F2.to_text(cs), F2.ends_text(cs), X.to_text2(cs)


def contigs_equal_fast(rfx, c, dl, dr, cs, tag):
    """contigs_equal of tests/test_gpu_fixing2.py on the vectorised packer"""
    packed_equals_fast(rfx, c, [x[0] for x in cs], tag)
    assert np.array_equal(dl[:c.n].cpu().numpy(), np.array([x[1] for x in cs], np.int32)), (tag, "left")
    assert np.array_equal(dr[:c.n].cpu().numpy(), np.array([x[2] for x in cs], np.int32)), (tag, "right")


@pytest.mark.parametrize("n", FIX2_SIZES)
def test_fix2_contigs_and_all_three_texts_with_a_third_dropped_in_every_tile(rfx, n):
    """k_fx2_cat_sizes' keep / words through exclusive_scan2_u32_to_u64 over 1, 2, 3 and 66 tiles (rank and woff out of step behind
    the first dropped contig), pk_find over woff and toff past 4,096, the text's exclusive_scan_u64 on two levels, idx 9,999 -> 10,000
    (270,000 records): fixing2_model.contigs, to_text, ends_text and extend_model.to_text2"""
    r = fix2_records(n)
    cs, text, ends, text2 = fix2_model(r)
    assert 0 < len(cs) < n
    c, dl, dr = rfx.fix2_contigs(rfx.dyn_pack(r), TF2.cparams(rfx, F2.default_params(FIX2_MAX_K)))
    contigs_equal_fast(rfx, c, dl, dr, cs, ("fix2 contigs", n))
    got_text, got_ends = TF2.both_texts(rfx, c, dl, dr)
    same_text(got_text, text, ("05FixingAgain", n))
    same_text(got_ends, ends, ("06ContigEnds", n))
    same_text(TX.text2_of(rfx, c), text2, ("09ExtendAgain", n))


def fix2_chain_rows():
    """contig_rows of tests/test_gpu_fixing.py with the 30-base keys 04Fixing writes: 5,000 contigs cut from one genome so that
    neighbours overlap and the loop merges them"""
    n, mk, _ = FIX2_CHAIN
    rng = np.random.default_rng(5005)
    g = strings_of(rng.integers(0, 4, 60 * n + 4 * mk + 200, dtype=np.uint8), np.array([0, 60 * n + 4 * mk + 200]))[0]
    rows, pos = [], 0
    for _ in range(n):
        L = 2 * mk + int(rng.integers(0, 91))
        c = g[pos:pos + L]
        pos += int(rng.integers(20, 60))
        m = int(rng.integers(1, 3))
        key, ext = (c[:F2.KEY], c[F2.KEY:]) if m == 1 else (c[L - F2.KEY:], c[:L - F2.KEY])
        rows.append(f"{key},{m}|{int(rng.choice(TF.MARK))}|{int(rng.choice(TF.MARK))},{ext}")
    return rows


def fix2_chain_want():
    """fixing2_model.run_stages on fix2_chain_rows with max_iteration = 1 -> (the records behind the last round, text, ends text)"""
    def make():
        n, mk, P = FIX2_CHAIN
        recs, passes, cs, text, ends = F2.run_stages(fix2_chain_rows(), F2.default_params(mk, max_iteration=1), P)
        return passes[-1], text, ends
    return want(("fix2 chain",), make)


def test_fix2_run_on_5000_records(rfx):
    """rfx_dev_fix2_run's rounds on more than one scan tile of records, then the contigs and both texts of what it leaves, and the host
    form: fixing2_model.run_stages"""
    n, mk, P = FIX2_CHAIN
    rows = fix2_chain_rows()
    last, text, ends = fix2_chain_want()
    cp = TF2.cparams(rfx, F2.default_params(mk, max_iteration=1))
    b = rfx.fix2_binarize(*upload(lines(rows)))
    assert b.n == n > TILE
    out = rfx.fix2_run(b, P, cp)
    equals_fast(rfx, out, host_dyn(last), "fix2 run")
    c, dl, dr = rfx.fix2_contigs(out, cp)
    contigs_equal_fast(rfx, c, dl, dr, F2.contigs(last, dict(max_k=mk)), "fix2 run, contigs")
    got_text, got_ends = TF2.both_texts(rfx, c, dl, dr)
    same_text(got_text, text, "fix2 run, 05FixingAgain")
    same_text(got_ends, ends, "fix2 run, 06ContigEnds")
    host = rfx.fix2_text("".join(lines(rows)).encode(), P, cp)
    assert (host[0].decode(), host[1].decode()) == (text, ends), "fix2 run, host form"


# ---- B. 07EndExtend ------------------------------------------------------------------------------------------------------------------------
ENDEXT_COUNTS = (4095, 4096, 4097)
ENDEXT_MAX_K = 71                                                  # 142: no contig of 62..140 bases is kept without a consensus
ENDEXT_SORT_CASES = {"top digit": (300, 0), "one long bucket": (300, 3000)}      # contigs, rows on the one crowded contig


def endext_input(n, crowded=0, pairs=3):
    """n contigs of 62..140 bases and, in front of them, one of 1 base and one of none (no rows of the output and no index: nidx and
    opos part from the contig number); per contig 0..pairs - 1 left and right rows of 2..60 / 1..60 bases, repeat markers on every
    9th (left) and 11th (right), four rows that name unknown contigs (their key is the contig count), `crowded` rows on contig 7; the
    rows permuted -> (contigs, rows)"""
    rng = np.random.default_rng(2400 + n + crowded)
    contigs = TE.make_contigs(rng, [1, 0] + [int(x) for x in rng.integers(62, 141, n - 2)], lr=[(int(a), int(b)) for a, b in rng.choice(MARK, (97, 2))])
    rows = []
    for i, c in enumerate(contigs[2:]):
        for _ in range(int(rng.integers(0, pairs))):
            rows.append(TE.left_row(rng, c, int(rng.integers(2, 61))))
            rows.append(TE.right_row(rng, c, int(rng.integers(1, 61))))
        if i % 9 == 4:
            rows += [f"{c[0]}\t0\t*\tL"] * 2
        if i % 11 == 6:
            rows += [f"{c[0]}\t0\t*\tR"] * 2
    truth = TF.rand_seq(rng, 60)
    for _ in range(crowded):
        cnt = int(rng.integers(1, 61))
        rows.append(TE.right_row(rng, contigs[7], cnt, TF.rand_seq(rng, 30) + truth[:cnt]))
    rows += [f"Contig_62_0_0_{n + j}\t1\t5S30M\t" + "A" * 35 for j in (0, 1, 5, 1000)]
    return contigs, [rows[i] for i in rng.permutation(len(rows))]


def set_equals_fast(rfx, s, cs, tag):
    """set_equals of tests/test_gpu_extend.py on the vectorised packer"""
    packed_equals_fast(rfx, s.set, [c["bases"] for c in cs], (tag, "bases"))
    got = s.host()
    for a in s.ARRAYS:
        assert np.array_equal(got[a], np.array([c[a] for c in cs], got[a].dtype)), (tag, a)


def device_set_from(contigs, cons, max_k):
    """endext_model.device_set with the consensus given (the model's pile-up, 2.6 s for 4,097 contigs, then runs once a case)"""
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


def endext_equals(rfx, contigs, rows, max_k, tag, whole_model=True):
    """stage_equals_model of tests/test_gpu_endext.py on the vectorised packer: the consensus sets and flags, the spliced set with its
    arrays, the text, and the host form against endext_model (whole_model: against run_text, the model's own second pile-up, too)
    -> the text"""
    c, dl, dr = TE.dev_contigs(rfx, contigs)
    wanted = want(("endext consensus",) + tuple(tag), lambda: E.device_consensus(contigs, rows))
    cons = rfx.endext_consensus(c, dl, dr, *TE.rows_up(rows))
    packed_equals_fast(rfx, cons.left, [w[0] for w in wanted], (tag, "left consensus"))
    packed_equals_fast(rfx, cons.right, [w[1] for w in wanted], (tag, "right consensus"))
    assert cons.flags[:c.n].cpu().tolist() == [w[2] for w in wanted], (tag, "flags")
    recs = device_set_from(contigs, wanted, max_k)
    assert len(contigs) > 1000 or recs == E.device_set(contigs, rows, max_k)
    s = rfx.endext_contigs(c, dl, dr, cons, max_k)
    set_equals_fast(rfx, s, recs, (tag, "spliced"))
    t, n = rfx.endext_to_text(s)
    text = text_from(t, n)
    ctext = "".join(f"{i},{b}\n" for i, b in contigs)
    same_text(text, E.set_text(recs), (tag, "text"))
    if whole_model:
        same_text(text, want(("endext text",) + tuple(tag), lambda: E.run_text(ctext, rows, max_k)), (tag, "the string model's text"))
    same_text(rfx.endext_text(ctext.encode(), "".join(r + "\n" for r in rows).encode(), max_k).decode(), text, (tag, "host form"))
    return text


@pytest.mark.parametrize("n", ENDEXT_COUNTS)
def test_endext_with_the_scans_over_contigs_on_one_and_two_tiles(rfx, n):
    """offl / offr, nidx / opos, woff, toff and the off of ee_contigs_from_rows over 4,095, 4,096 and 4,097 contigs, pk_find over woff
    and toff past 4,096, the row key one bit wider from 4,096 on, the output in the order of the ID strings with kept and dropped
    contigs mixed all along it"""
    contigs, rows = endext_input(n)
    text = endext_equals(rfx, contigs, rows, ENDEXT_MAX_K, ("endext", n), whole_model=n == ENDEXT_COUNTS[-1])
    assert 0 < text.count("\n") < n - 2


@pytest.mark.parametrize("case", sorted(ENDEXT_SORT_CASES))
def test_endext_row_sort_on_the_top_digit_path_and_behind_its_refusal(rfx, case):
    """more than 255 contigs and more than 2,048 rows: sort_pairs leaves k_sort_small for the top-digit path; with 3,000 rows on one
    contig a bucket exceeds a tile, the top digit refuses and the LSD passes sort"""
    n, crowded = ENDEXT_SORT_CASES[case]
    contigs, rows = endext_input(n, crowded, pairs=9)
    assert n > 255 and len(rows) > SORT_SMALL
    endext_equals(rfx, contigs, rows, 31, ("endext", case))


# ---- C. 08Extend / 09ExtendAgain -----------------------------------------------------------------------------------------------------------
EXT_ROWS = (4096, 4097, 8193)
EXT_MAX_K = 40                                                     # rows of fewer than 80 characters are dropped
EXT_CHAIN = (4300, 31, 3, 1)                                       # contigs, max_k, P, max_iteration of the chain


def ext_rows(n):
    """n rows of 07EndExtend: contigs of 62..140 bases, ends of 0..6 bases, the four flag patterns in turn (a flagged end holds its
    literal besides)"""
    rng = np.random.default_rng(2500 + n)
    return [TX.end_row(rng, i, int(rng.integers(62, 141)), int(rng.integers(0, 7)), int(rng.integers(0, 7)), bool(i & 1), bool(i & 2)) for i in range(n)]


def ext_offsets(rows, p):
    """-> per row: kept, and the three quantities rfx_dev_ext_contig_ends scans: its end 31-mers (ll + rl), 1, the words of its cut contig"""
    kept, k, w = [], [], []
    for row in rows:
        (_, _, _, _, ll, rl, _), seq = X.parse_row(row)
        ok = len(seq) >= 2 * p["max_k"]
        kept.append(ok)
        k.append(ll + rl if ok else 0)
        w.append((len(seq) - ll - rl - (X.FIX_K - 1) + 31) // 32 if ok else 0)
    return np.array(kept), np.array(k), np.array(w)


def kmer_values_np(kmers):
    """value_of of tests/test_gpu_fixing.py for a list of 31-mers: 62 bits, the first base in bits 61..60"""
    if not kmers:
        return np.zeros(0, np.int64)
    c = codes_of(kmers).reshape(len(kmers), X.FIX_K).astype(np.uint64)
    return np.bitwise_or.reduce(c << (np.uint64(2) * np.arange(X.FIX_K - 1, -1, -1, dtype=np.uint64)), axis=1).astype(np.int64)


@pytest.mark.parametrize("n", EXT_ROWS)
def test_ext_set_and_contig_ends_with_dropped_rows_in_every_tile(rfx, n):
    """ex_rows_plan's scan and the three offset arrays of ex_contig_ends (koff, loff, woff, each crossing 4,096 at another contig)
    with pk_find over them, from the text and from the view with the literals in flags: extend_model.device_set, the long records
    and the 31-mers in emission order"""
    rows = ext_rows(n)
    p = X.default_params(EXT_MAX_K, max_iteration=0)
    prm = TF.cparams(rfx, p)
    longs, kmers = X.contig_ends(X.binarize(rows, p), p)
    assert 0 < len(longs) < n and len(kmers) > TILE
    s_text = rfx.ext_from_text(*upload(lines(rows)), prm)
    set_equals_fast(rfx, s_text, X.device_set(rows, p, False), ("ext from text", n))
    s_dev = TX.dev_set(rfx, X.device_set(rows, p, True))
    values = kmer_values_np(kmers)
    for view, s in (("text", s_text), ("flags", s_dev)):
        lg, d_k, nk = rfx.ext_contig_ends(s, prm)
        equals_fast(rfx, lg, host_dyn(longs), ("ext long", n, view))
        assert nk == len(kmers) and np.array_equal(d_k[:nk].cpu().numpy(), values), ("ext 31-mers", n, view)


def ext_chain_rows():
    """genome_rows of tests/test_gpu_extend.py with ends of 0..8 bases: 4,300 contigs cut from one genome, the ends reaching into their
    neighbours, a flagged end on every fifth and seventh"""
    n, mk, _, _ = EXT_CHAIN
    rng = np.random.default_rng(4300)
    g = strings_of(rng.integers(0, 4, 150 * n + 4 * mk + 800, dtype=np.uint8), np.array([0, 150 * n + 4 * mk + 800]))[0]
    rows, pos = [], 310
    for i in range(n):
        L = 2 * mk + int(rng.integers(0, 60))
        ll, rl = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        rows.append(TX.end_row(rng, i, L, ll, rl, fl=i % 5 == 1, fr=i % 7 == 2, contig=g[pos:pos + L], le=g[pos - ll:pos], re=g[pos + L:pos + L + rl]))
        pos += L + int(rng.integers(-20, 40))
    return rows


def ext_chain_want():
    """extend_model.run_stages and run2_stages on ext_chain_rows -> (the set behind 08's last pass, its text, 09's contigs, its text)"""
    def make():
        n, mk, P, it = EXT_CHAIN
        p = X.default_params(mk, max_iteration=it)
        passes = X.run_stages(ext_chain_rows(), p, P, order="sorted")[3]
        text = X.to_text(passes[-1])
        _, _, cs, text2 = X.run2_stages(text.splitlines(), p, P)
        return passes[-1], text, cs, text2
    return want(("ext chain",), make)


def test_ext_run_and_09_on_4300_contigs(rfx):
    """rfx_dev_ext_run on more contigs than a scan tile, its text and the host form, then 09ExtendAgain on the resident set
    (fix2_run -> fix2_contigs -> ext2_to_text) and from the text: extend_model.run_stages and run2_stages"""
    n, mk, P, it = EXT_CHAIN
    rows = ext_chain_rows()
    last, text, cs, text2 = ext_chain_want()
    prm = TF.cparams(rfx, X.default_params(mk, max_iteration=it))
    s = rfx.ext_from_text(*upload(lines(rows)), prm)
    assert s.n == n > TILE
    out = rfx.ext_run(s, P, prm)
    equals_fast(rfx, out, host_dyn(last), "ext run")
    same_text(TF.text_of(rfx, out), text, "08Extend")
    same_text(rfx.ext_text("".join(lines(rows)).encode(), P, prm).decode(), text, "08Extend, host form")
    c, dl, dr = rfx.fix2_contigs(rfx.fix2_run(out, P, prm), prm)
    packed_equals_fast(rfx, c, [x[0] for x in cs], "09 contigs")
    same_text(TX.text2_of(rfx, c), text2, "09ExtendAgain")
    same_text(rfx.ext2_text(text.encode(), P, prm).decode(), text2, "09ExtendAgain, host form")


# ---- D. the end mapper ---------------------------------------------------------------------------------------------------------------------
MAP_CONTIG_COUNTS = (512, 513, 98_305)                             # m = 4 contigs: 2,048 (k_sort_small), 2,052 (top digit), 393,220 (two levels)
MAP_PLANTED = 1500                                                 # contigs with a read over each end, on both strands
MAP_SHARED = 64                                                    # contigs that begin with the first 45 bases of another one
MAP_READ = 40                                                      # bases of a read of the grid-cap cases
MAP_SEED = MP.DEFAULTS["seed"]


def seed_table(ends, seed):
    """{the seed of an end: [its position in ends]}, in end order"""
    table = {}
    for j, (_, _, T, side, _) in enumerate(ends):
        if len(T) >= seed:
            table.setdefault(T[:seed] if side == 0 else T[len(T) - seed:], []).append(j)
    return table


def hits_indexed(contigs, reads, seed=21, min_overlap=31, max_mismatch=2):
    """map_model.hits with the ends found through a dict from seed to ends, not by trying every end on every read: the same placements
    by the same map_model.place, rows in the model's order (read, strand, end, offset)"""
    ends = MP.ends_of(contigs)
    table = seed_table(ends, seed)
    out = []
    for ri, read in enumerate(reads):
        fw = MP.norm(read)
        for strand, r in enumerate((fw, MP.revcomp(fw))):
            cand = sorted({(j, off) for off in range(len(r) - seed + 1) for j in table.get(r[off:off + seed], ())})
            for j, off in cand:
                e, name, T, side, whole = ends[j]
                got = MP.place(r, T, side, whole, off, seed, min_overlap, max_mismatch)
                if got:
                    out.append((ri, e, strand, off, got[0], got[1], got[2], name, r, len(T)))
    return out


def map_contigs(n):
    """n contigs of 62..140 bases (numpy-made), MAP_SHARED of them beginning with the first 45 bases of a contig far away, so that equal
    seeds sit in table entries far apart -> [(ID, bases)]"""
    rng = np.random.default_rng(2600 + n)
    ln = rng.integers(62, 141, n)
    off = offsets_of(ln)
    codes = rng.integers(0, 4, off[-1], dtype=np.uint8)
    src = rng.choice(n, min(MAP_SHARED, n // 4), replace=False)
    dst = (src + n // 2) % n
    for a, b in zip(src, dst):
        codes[off[b]:off[b] + 45] = codes[off[a]:off[a] + 45]
    seqs = strings_of(codes, off)
    lr = rng.integers(-3, 4, (n, 2))
    return [(f"Contig_{len(s)}_{int(l)}_{int(r)}_{i}", s) for i, (s, (l, r)) in enumerate(zip(seqs, lr))]


def map_reads(contigs):
    """reads of 100 bases over both ends of MAP_PLANTED contigs drawn from all over the set (the first and the last among them, and
    the contigs that share a seed, whose left read stays inside the shared bases), each on one strand; one read in 4 with a changed base in its overlap; 200 random reads"""
    n = len(contigs)
    rng = np.random.default_rng(2700 + n)
    first = {}
    for i, (_, b) in enumerate(contigs):
        first.setdefault(b[:MAP_SEED], []).append(i)
    shared = {i for v in first.values() if len(v) > 1 for i in v}
    pick = sorted(set(rng.choice(n, min(MAP_PLANTED, n), replace=False).tolist()) | {0, 1, n // 2, n - 2, n - 1} | shared)
    reads = []
    for j, i in enumerate(pick):
        b = contigs[i][1]
        l = MP.rand_seq(rng, 1 + j % 37) + b[:40 if i in shared else 100]      # (inside the shared 45 bases: a row on both contigs)
        r = b[-100:] + MP.rand_seq(rng, 1 + j % 29)
        if j % 4 == 0:
            l = l[:-5] + "ACGT"[("ACGT".index(l[-5]) + 1) % 4] + l[-4:]
        reads += [l if j % 2 else MP.revcomp(l), MP.revcomp(r) if j % 3 else r]
    reads += [MP.rand_seq(rng, 100) for _ in range(200)]
    return [reads[i] for i in rng.permutation(len(reads))]


def map_equals(rfx, contigs, dw, dn, wpr, n_reads, hs, tag, host_reads=None):
    """check of tests/test_gpu_map.py with the expected rows given: rfx_dev_map_ends field by field, rfx_dev_map_to_text byte for byte
    with its row offsets, and (host_reads) rfx_map_text"""
    c, dl, dr = TE.dev_contigs(rfx, contigs)
    p = rfx.map_params()
    got = rfx.map_ends(c, dl, dr, dw, dn, n_reads, wpr, p)
    wanted, g = MP.fields(hs), got.host()
    assert got.n == len(hs), (tag, got.n, len(hs))
    for a in got.ARRAYS:
        if not np.array_equal(g[a], wanted[a]):
            i = int(np.flatnonzero(g[a] != wanted[a])[0])
            raise AssertionError((tag, a, "first difference at row", i, g[a][i:i + 8].tolist(), wanted[a][i:i + 8].tolist()))
    t, ln, off = rfx.map_to_text(c, dl, dr, dw, dn, wpr, got)
    rows = [MP.row_of(h) + "\n" for h in hs]
    same_text(text_from(t, ln), "".join(rows), (tag, "text"))
    assert np.array_equal(off.cpu().numpy(), offsets_of(np.array([len(r) for r in rows], np.int64))), (tag, "row offsets")
    if host_reads is not None:
        same_text(rfx.map_text(MP.contig_text(contigs).encode(), host_reads, p).decode(), "".join(rows), (tag, "host form"))


@pytest.mark.parametrize("n", MAP_CONTIG_COUNTS)
def test_map_with_the_seed_table_sorted_by_each_path(rfx, n):
    """the seed table of 4 n pairs through k_sort_small (2,048), the top-digit path (2,052) and two MSD levels (393,220), the reads'
    binary search over it, equal seeds far apart: map_model's placements through a dict of the seeds"""
    from tests.test_gpu_map import dev_reads
    contigs = map_contigs(n)
    reads = map_reads(contigs)
    hs = hits_indexed(contigs, reads)
    assert len(hs) >= (len(reads) - 200) * 9 // 10
    dw, dn, wpr = dev_reads(reads)
    map_equals(rfx, contigs, dw, dn, wpr, len(reads), hs, ("map contigs", n), host_reads=[r.encode() for r in reads])


def window_keys(codes, k):
    """[n, L] base codes -> ([n, L - k + 1] forward keys, the keys of the reverse complements): 2 bits a base, the last in the lowest"""
    n, L = codes.shape
    W = L - k + 1
    fw, rc = np.zeros((n, W), np.uint64), np.zeros((n, W), np.uint64)
    c = codes.astype(np.uint64)
    for j in range(k):
        fw |= c[:, j:j + W] << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - c[:, j:j + W]) << np.uint64(2 * j)
    return fw, rc


def pack_codes(codes, lens, wpr, junk=None):
    """the 2-bit read store of [n, L] base codes with lengths lens, in one step: (words uint64 [n, wpr], lengths uint32); junk (an rng):
    every bit behind a read's last base is random"""
    n, L = codes.shape
    full = junk.integers(0, 4, (n, 32 * wpr), dtype=np.uint8) if junk is not None else np.zeros((n, 32 * wpr), np.uint8)
    at = np.arange(L) < np.asarray(lens)[:, None]
    full[:, :L][at] = codes[at]
    q = full.reshape(n * wpr * 8, 4)
    b = np.ascontiguousarray((q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3], np.uint8)
    return b.view(">u8").astype(np.uint64).reshape(n, wpr), np.asarray(lens, np.uint32)


def upload_reads(words, lens):
    import torch
    dw, dn = torch.from_numpy(words.view(np.int64).reshape(-1).copy()).cuda(), torch.from_numpy(lens.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    return dw, dn


def grid_cap_reads(cus, extra):
    """5 cus 256 + extra random reads of 40 bases against three contigs (130, 450 and 95 bases); planted on a contig end: every 997th
    read, every third of the last 300, and every read from 5 cus 256 on (the reads a block takes on its second trip) but each fifth
    -> (contigs, codes [n, 40], the planted read numbers)"""
    cap = 5 * cus * 256
    n = cap + extra
    rng = np.random.default_rng(2800 + extra)
    contigs = [(f"Contig_{L}_{i - 1}_{2 - i}_{i}", MP.rand_seq(rng, L)) for i, L in enumerate((130, 450, 95))]
    codes = rng.integers(0, 4, (n, MAP_READ), dtype=np.uint8)
    planted = sorted(set(range(500, n, 997)) | set(range(n - 300, n, 3)) | {i for i in range(cap, n) if (i - cap) % 5 != 4})
    for j, i in enumerate(planted):
        b = contigs[j % 3][1]
        over = 1 + j % 9
        r = MP.rand_seq(rng, over) + b[:MAP_READ - over] if j % 2 else b[-(MAP_READ - over):] + MP.rand_seq(rng, over)
        codes[i] = codes_of([MP.revcomp(r) if j % 4 < 2 else r])
    return contigs, codes, planted


def hits_prefiltered(contigs, codes, seed=MAP_SEED):
    """map_model.hits on reads of one length given as codes: only a read that holds the seed of an end, or the reverse complement of
    one, in some window can have a row (the model itself skips an end whose seed the oriented read does not contain), so the model
    runs on those reads alone, found with numpy, and its read numbers are mapped back"""
    keys = []
    for _, _, T, side, _ in MP.ends_of(contigs):
        if len(T) >= seed:
            s = codes_of([T[:seed] if side == 0 else T[len(T) - seed:]])[None, :]
            keys += [int(x[0, 0]) for x in window_keys(s, seed)]
    fw, _ = window_keys(codes, seed)
    cand = np.flatnonzero(np.isin(fw, np.array(sorted(set(keys)), np.uint64)).any(axis=1))
    reads = strings_of(codes[cand].reshape(-1), np.arange(len(cand) + 1) * codes.shape[1])
    return [(int(cand[h[0]]),) + h[1:] for h in MP.hits(contigs, reads, seed=seed)]


@pytest.mark.parametrize("extra", (0, 1, 257))
def test_map_reads_around_the_grid_cap(rfx, extra):
    """k_mp_scan's grid is capped at 5 blocks a CU: with 5 CUs 256 reads every block makes one trip, with one more the first block
    makes a second, with 257 more the second block too; rows in the last 300 reads and in the second trip's, hoff's scan above
    262,144 on 256 CUs: map_model.hits on the reads that hold a seed"""
    cus = device_cus()
    cap = 5 * cus * 256
    contigs, codes, planted = grid_cap_reads(cus, extra)
    n = len(codes)
    hs = hits_prefiltered(contigs, codes)
    with_rows = {h[0] for h in hs}
    assert n == cap + extra and any(i >= n - 300 for i in with_rows) and (extra == 0 or any(i >= cap for i in with_rows))
    assert len(with_rows) >= len(planted) * 9 // 10
    words, lens = pack_codes(codes, np.full(n, MAP_READ), 2, junk=np.random.default_rng(extra))
    dw, dn = upload_reads(words, lens)
    host = (NUC[codes.reshape(-1)], np.arange(n + 1, dtype=np.int64) * MAP_READ) if extra == 257 else None
    map_equals(rfx, contigs, dw, dn, 2, n, hs, ("map reads", n), host_reads=host)


# ---- E. the mercy stage ----------------------------------------------------------------------------------------------------------------------
MERCY_K = {4096: 8, 4097: 11, "cap": 13, "cap + 1": 15, 270_000: 12}
MERCY_LARGE = 270_000
MERCY_WAVES_PER_CU = 8 * 4                                         # mc_plan: 8 blocks a CU, MC_WAVES waves each, a wave per read
MERCY_ROWS = (340_000, 70_000, 6000, 15)                           # distinct count rows, repeats, rows of another length, k
MERCY_ROW_READS = 3000


def mercy_reads(n, k):
    """n reads of at most 31 bases as codes: half of them with two windows planted solid whose gap is kept, a third of 16 bases (which
    FastqTuple2Dataset's filter drops whatever they hold), a sixth with one planted window; the last read is of the first kind
    -> (codes [n, 32], lengths, the solid keys ascending)"""
    rng = np.random.default_rng(2900 + n + k)
    u = rng.random(n)
    kind = np.where(u < 0.5, 0, np.where(u < 5.0 / 6, 1, 2))
    kind[n - 1] = 0
    lo = max(17, k + 9)
    lens = np.where(kind == 1, 16, rng.integers(lo, 32, n))
    codes = rng.integers(0, 4, (n, 32), dtype=np.uint8)
    codes[np.arange(32) >= lens[:, None]] = 0
    W = lens - k + 1                                                # windows of a read
    a = rng.integers(0, 3, n)
    gmax = np.minimum(W - 2 - a, k - 2)                             # a kept gap: 1 .. k - 2 windows, the second hit inside the read
    b = a + 2 + rng.integers(0, np.maximum(gmax, 1))
    fw, rc = window_keys(codes, k)
    canon = np.minimum(fw, rc)
    rows = np.arange(n)
    two, one = kind == 0, kind == 2
    solid = np.unique(np.concatenate([canon[rows[two], a[two]], canon[rows[two], b[two]], canon[rows[one], a[one]]]))
    return codes, lens.astype(np.int64), solid


def mercy_np(codes, lens, k, solid, front_clip=0, end_clip=0):
    """mercy_model.mercy_kmers on reads given as codes (zeros behind a read's last base), the solid set as ascending canonical keys
    -> (the mercy k-mers' keys in output order, the number each read gives)"""
    n, L = codes.shape
    lens = np.asarray(lens, np.int64)
    fw, rc = window_keys(codes, k)
    canon = np.minimum(fw, rc)
    W = canon.shape[1]
    p = np.arange(W)
    none = (lens - k - end_clip + 1 <= 0) | (front_clip > lens) | (lens - 15 - end_clip <= 1)
    if L >= 32:
        none |= (lens >= 32) & (codes[:, :31] == 0).all(axis=1)
    valid = (p >= front_clip) & (p <= (lens - end_clip - k)[:, None]) & ~none[:, None]
    at = np.searchsorted(solid, canon)
    hit = valid & (solid[np.minimum(at, len(solid) - 1)] == canon) if len(solid) else np.zeros_like(valid)
    before = np.maximum.accumulate(np.where(hit, p, -1), axis=1)
    after = np.minimum.accumulate(np.where(hit, p, 1 << 30)[:, ::-1], axis=1)[:, ::-1]
    g = after - before - 1
    kept = ~hit & (before >= 0) & (after < (1 << 30)) & ~((g >= k - 1) & (g <= k + 1))
    return canon[kept], kept.sum(axis=1)


def kmer_codes(keys, k):
    """keys -> [n, k] base codes"""
    keys = np.asarray(keys, np.uint64)
    return ((keys[:, None] >> (np.uint64(2) * np.arange(k - 1, -1, -1, dtype=np.uint64))) & np.uint64(3)).astype(np.uint8)


def kmer_strings(keys, k):
    return strings_of(kmer_codes(keys, k).reshape(-1), np.arange(len(keys) + 1) * k)


def mercy_text_np(keys, k):
    """the rows `KMER,1` of the keys"""
    rows = np.empty((len(keys), k + 3), np.uint8)
    rows[:, :k], rows[:, k:] = NUC[kmer_codes(keys, k)], np.frombuffer(b",1\n", np.uint8)
    return rows.tobytes().decode()


def mercy_keys_of(kmers):
    return np.array([MC.key_of(s) for s in kmers], np.uint64)


def mercy_sizes(cus):
    cap = MERCY_WAVES_PER_CU * cus
    return [(4096, MERCY_K[4096]), (4097, MERCY_K[4097]), (cap, MERCY_K["cap"]), (cap + 1, MERCY_K["cap + 1"])]


def dev_solid(solid):
    import torch
    d = torch.from_numpy(np.concatenate([solid, np.zeros(1, np.uint64)]).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return d


def mercy_equals(rfx, codes, lens, k, solid, want_keys, tag):
    words, ln32 = pack_codes(codes, lens, 1, junk=np.random.default_rng(k))
    dw, dn = upload_reads(words, ln32)
    got = rfx.mercy_kmers(dev_solid(solid), len(solid), dw, dn, len(lens), 1, k)
    assert got.n == len(want_keys), (tag, got.n, len(want_keys))
    g = got.host()
    if not np.array_equal(g, want_keys):
        i = int(np.flatnonzero(g != want_keys)[0])
        raise AssertionError((tag, "first key that differs", i, g[i:i + 4].tolist(), want_keys[i:i + 4].tolist()))
    t, n, off = rfx.mercy_to_text(got.keys, got.n, k)
    same_text(text_from(t, n), mercy_text_np(want_keys, k), (tag, "text"))
    assert np.array_equal(off.cpu().numpy(), np.arange(len(want_keys) + 1) * (k + 3)), (tag, "row offsets")


@pytest.mark.parametrize("case", range(4))
def test_mercy_reads_over_two_scan_tiles_and_a_second_trip_of_the_grid(rfx, case):
    """4,096 / 4,097 reads: plan.off's scan on one and two tiles; 32 reads a CU and one more: the last size at which k_mc_scan's loop makes one
    trip and the first at which the first wave makes a second, in the counting and in the fill pass; a third of the reads give
    nothing, the last read gives k-mers: mercy_model.mercy_kmers, all three entry points"""
    n, k = mercy_sizes(device_cus())[case]
    codes, lens, solid = mercy_reads(n, k)
    reads = strings_of(codes.reshape(-1), np.arange(n + 1) * 32)
    reads = [r[:m] for r, m in zip(reads, lens.tolist())]
    kmers = MC.mercy_kmers(reads, k, 0, 0, set(kmer_strings(solid, k)))
    per_read = mercy_np(codes, lens, k, solid)[1]
    assert per_read[n - 1] > 0 and per_read.sum() == len(kmers) and every_tile_has(per_read == 0) and every_tile_has(per_read > 0)
    want_keys = mercy_keys_of(kmers)
    mercy_equals(rfx, codes, lens, k, solid, want_keys, ("mercy", n, k))
    rows = "".join(f"{s},2\n" for s in kmer_strings(solid[::-1], k))
    host = rfx.mercy_text(rows.encode(), (NUC[codes[np.arange(32) < lens[:, None]]], offsets_of(lens)), k)
    same_text(host.decode(), "".join(f"{s},1\n" for s in kmers), ("mercy", n, k, "host form"))


def test_mercy_on_270000_reads(rfx):
    """66 tiles of counts with zeros all over them, every wave on many trips: the numpy statement of mercy_model.mercy_kmers"""
    n, k = MERCY_LARGE, MERCY_K[MERCY_LARGE]
    codes, lens, solid = mercy_reads(n, k)
    want_keys, per_read = mercy_np(codes, lens, k, solid)
    assert n > LANE_WINDOW and per_read[n - 1] > 0 and per_read[MERCY_WAVES_PER_CU * device_cus():].any()
    mercy_equals(rfx, codes, lens, k, solid, want_keys, ("mercy", n, k))


def mercy_count_rows():
    """416,000 count rows in random order: 340,000 random 15-mers, 70,000 repeats of them with another count, 6,000 rows of 14 and 16
    letters; and 3,000 reads of 60 bases, each with windows 2 and 2 + g solid (the rows hold those k-mers, as they read or turned
    round) -> (rows, reads)"""
    distinct, repeats, foreign, k = MERCY_ROWS
    rng = np.random.default_rng(2950)
    rc = np.zeros((MERCY_ROW_READS, 60), np.uint8)
    rc[:] = rng.integers(0, 4, rc.shape)
    reads = strings_of(rc.reshape(-1), np.arange(MERCY_ROW_READS + 1) * 60)
    planted = []
    for i, r in enumerate(reads):
        for p in (2, 4 + i % 40):
            s = r[p:p + k]
            planted.append(MC.canon(s) if i % 2 else s)
    own = strings_of(rng.integers(0, 4, k * (distinct - len(planted)), dtype=np.uint8), np.arange(distinct - len(planted) + 1) * k) + planted
    rows = [f"{s},{2 + i % 7}\n" for i, s in enumerate(own)]
    rows += [f"{own[i]},{9 + j % 5}\n" for j, i in enumerate(rng.choice(len(own), repeats).tolist())]
    fl = rng.choice([k - 1, k + 1], foreign)
    rows += [f"{s},3\n" for s in strings_of(rng.integers(0, 4, int(fl.sum()), dtype=np.uint8), offsets_of(fl))]
    return [rows[i] for i in rng.permutation(len(rows))], reads


def test_mercy_host_form_sorts_400000_count_rows_with_duplicates(rfx):
    """rfx_mercy_text: the rows' keep scan over 102 tiles with zeros in each, sort_pairs on 410,000 keys (two MSD levels), k_mc_heads
    and scan_keep dropping the repeats: mercy_model.solid_set and mercy_kmers"""
    k = MERCY_ROWS[3]
    rows, reads = mercy_count_rows()
    solid = MC.solid_set(rows, k)
    kmers = MC.mercy_kmers(reads, k, 0, 0, solid)
    assert len(rows) - MERCY_ROWS[2] > SORT_TWO_LEVELS and len(solid) < len(rows) - MERCY_ROWS[2] - MERCY_ROWS[1] // 2 and len(kmers) > MERCY_ROW_READS
    got = rfx.mercy_text("".join(rows).encode(), [r.encode() for r in reads], k)
    same_text(got.decode(), "".join(f"{s},1\n" for s in kmers), "mercy host form")


# ---- F. poisoned allocations ---------------------------------------------------------------------------------------------------------------
def test_everything_again_with_every_allocation_poisoned(tmp_path):
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is 0xA5 before the library uses it.  A child process (the mask is read
    once per process), which takes what the slow string models gave -- the two chains, and the pile-ups of 07EndExtend this process
    has made by now -- from a file this process writes"""
    fix2_chain_want()
    ext_chain_want()
    path = tmp_path / "want.pickle"
    with open(path, "wb") as f:
        pickle.dump(_want, f)
    env = dict(os.environ, RFX_POISON="7", **{WANT_ENV: str(path)})
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
