"""The contig RC de-duplication on packed sets (rfx_dedup.hip) past the sizes where its launches change shape
(the fourth table).  Its own files stay inside one scan tile of contigs, inside k_sort_small and inside one
block of k_dd_select, and batch at most 66 merges; here pack / unpack / from-text / to-text run over 2,048 .. 8,193 and 270,000
contigs with dropped contigs in every tile, the marker sort leaves k_sort_small for the top-digit path and for two MSD levels, one
step of a round batches thousands of merges, an equal-31-mer run spans a sort tile, and marker rows are left over.

Every comparison is exact.  What is expected comes from oracle.dedup_contigs (one byte per base, no batching), from the numpy
statement of the layout (contig_words_np of tests/test_gpu_contig_scale.py) and from the Python statement of the text (text_of /
path_text of tests/test_gpu_dedup_packed.py, or the list forms below that tests/test_dedup_scale_inputs.py pins to them); never from
another entry point of the library.  tests/test_dedup_scale_inputs.py asserts on the CPU every condition on the inputs that the
tests here rely on."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests import test_gpu_dedup_packed as P
from tests.test_gpu_contig_scale import SORT_SMALL, SORT_TWO_LEVELS, TILE, LANE_WINDOW, contig_words_np, same_text   # noqa: F401
from tests.test_gpu_dedup_packed import E_CAP, FILL, OK, rc

pytestmark = pytest.mark.gpu

NUC = np.frombuffer(b"ACGT", np.uint8)
TO_T = bytes(b if chr(b) in "ACG" else ord("T") for b in range(256))      # what a packed contig reads back as


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


# ---- what the oracle gave, made once: in this process, or by the parent of the poisoned run ---------------------------------------------
WANT_ENV = "RFX_DEDUP_SCALE_WANT"                                  # a pickle of {key: oracle result} the parent process wrote
_want = {}


def want(key, make):
    if not _want and os.environ.get(WANT_ENV):
        with open(os.environ[WANT_ENV], "rb") as f:
            _want.update(pickle.load(f))
    if key not in _want:
        _want[key] = make()
    return _want[key]


# ---- the layout and the two texts without a Python statement per contig ---------------------------------------------------------------------
def rand_seq(rng, n):
    return NUC[rng.integers(0, 4, n)].tobytes().decode()


def as_t_fast(contigs):
    """[as_t(s) for s in contigs] of tests/test_gpu_dedup_packed.py: one translate over the joined letters"""
    text = "".join(contigs).encode().translate(TO_T).decode()
    off = np.concatenate([[0], np.cumsum([len(s) for s in contigs])]).tolist()
    return [text[a:b] for a, b in zip(off[:-1], off[1:])]


def headers_of(lengths, idx):
    return np.char.add(np.char.add(">Contig-", lengths.astype(str)), np.char.add("-", idx.astype(str))).tolist()


def text_of_fast(contigs, min_contig):
    """text_of of tests/test_gpu_dedup_packed.py for contigs below one line of 10,000,000 bases"""
    ln = np.array([len(s) for s in contigs], np.int64)
    assert len(ln) == 0 or ln.max() < P.LINE
    idx = np.flatnonzero(ln >= min_contig)
    if len(idx) == 0:
        return ""
    parts = [None] * (2 * len(idx))
    parts[0::2] = headers_of(ln[idx], idx)
    parts[1::2] = [contigs[i] for i in idx.tolist()]
    return "\n".join(parts) + "\n"


def path_text_fast(contigs, eol="\n", junk=True):
    """path_text of tests/test_gpu_dedup_packed.py for contigs of at most one line of 100 columns"""
    ln = np.array([len(s) for s in contigs], np.int64)
    assert len(ln) == 0 or ln.max() <= 100
    lines = [x for pair in zip(headers_of(ln, np.arange(len(ln))), contigs) for x in pair if x]
    return ("not a header" + eol + eol if junk else "") + "".join(x + eol for x in lines)


def raw_equals_fast(pk, contigs, tag):
    """raw_equals of tests/test_gpu_dedup_packed.py on the vectorised packer: words (every padding bit), word offsets, lengths"""
    words, word_off, length = pk.host()
    w, o, l = contig_words_np(contigs)
    assert pk.n == len(contigs), (tag, pk.n, len(contigs))
    assert np.array_equal(length, l), (tag, "len")
    assert np.array_equal(word_off, o), (tag, "word_off")
    assert words.shape == w.shape and np.array_equal(words, w), (tag, "words")


def same_list(got, wanted, tag):
    if got != wanted:
        i = next((j for j, (a, b) in enumerate(zip(got, wanted)) if a != b), min(len(got), len(wanted)))
        raise AssertionError((tag, len(got), len(wanted), "first contig that differs", i))


# ---- (a) the layout and the text over more than one tile ------------------------------------------------------------------------------------
SCAN_TILE = 2048                                                   # rfx_scan.hip: exclusive_scan_u64 (cw -> woff, sz -> toff) runs a second level above it
LAYOUT_SIZES = (2048, 2049, 4095, 4096, 4097, 8193)
LAYOUT_BIG = 270_000                                               # 132 tiles of contigs, 13 MB of text
LAYOUT_BIG_MAX = 70
MIN_CONTIGS = (0, 32, 500)
KEPT_AT = (9_999, 10_000, 99_999, 100_000)                         # the header grows by a column behind the first and the third


def layout_contigs(n):
    """n <= 8,193: lengths cycle through LENGTHS of tests/test_gpu_dedup_packed.py (0..1000 bases, N and lower case among the
    letters), the last one of 1,000 bases; 270,000: lengths 0..70 from the same letters, those on either side of a header-width step
    of 70 bases"""
    rng = np.random.default_rng(1600 + n)
    if n < LAYOUT_BIG:
        contigs = P.mixed_contigs(rng, n)
        contigs[n - 1] = contigs[P.LENGTHS.index(1000)]            # the last contig is kept: at 2,049, 4,097 and 8,193 it is a tile of its own
        return contigs
    alphabet = np.frombuffer(b"ACGTACGTACGTNacgtn", np.uint8)
    ln = rng.integers(0, LAYOUT_BIG_MAX + 1, n)
    ln[list(KEPT_AT)] = LAYOUT_BIG_MAX
    off = np.concatenate([[0], np.cumsum(ln)]).tolist()
    text = alphabet[rng.integers(0, len(alphabet), off[-1])].tobytes().decode()
    return [text[a:b] for a, b in zip(off[:-1], off[1:])]


@pytest.mark.parametrize("n", LAYOUT_SIZES + (LAYOUT_BIG,))
def test_pack_unpack_and_the_two_texts_over_more_than_one_tile(rfx, n):
    """cw -> woff of from-text and sz -> toff of to-text (exclusive_scan_u64: one level up to 2,048 contigs, two from 2,049 on) and
    pk_find over woff in k_dd_pack, k_dd_unpack, k_dd_text_fill and k_dd_out_bases on 1, 2, 3, 5 and 132 tiles of contigs, contigs
    dropped from the text in every tile, the header a column wider from idx 10,000 and 100,000 on: the raw words, offsets and
    lengths are the numpy packer's, unpack(pack(x)) = x with every letter that is not ACG read as T, and both texts are the Python
    statements"""
    contigs = layout_contigs(n)
    read_back = as_t_fast(contigs)
    pk = rfx.contigs_pack(contigs)
    raw_equals_fast(pk, contigs, ("pack", n))
    same_list(rfx.contigs_unpack(pk), read_back, ("unpack", n))
    for eol in ("\n", "\r\n"):
        text = P.path_text(contigs, eol) if n < LAYOUT_BIG else path_text_fast(contigs, eol)
        d_text, ln = P.on_device(text)
        raw_equals_fast(rfx.contigs_from_text_dev(d_text, ln), contigs, ("from_text", n, eol))
    for min_contig in MIN_CONTIGS if n < LAYOUT_BIG else MIN_CONTIGS[:2]:
        text, nc = P.device_text(rfx, pk, min_contig)
        same_text(text, P.text_of(read_back, min_contig) if n < LAYOUT_BIG else text_of_fast(read_back, min_contig), ("to_text", n, min_contig))
        assert nc == sum(1 for s in contigs if len(s) >= min_contig), (n, min_contig)


def test_exact_capacities_at_8193_contigs_and_one_short(rfx):
    """pack and from-text into a set of exactly the needs: OK and the numpy packer's arrays; one contig or one word short: RFX_E_CAP,
    the needs reported, every output byte (0xA5) as it was; the same for the text buffer, exact and one byte short"""
    import torch
    L, ctx = rfx.L, rfx.ctx
    contigs = layout_contigs(8193)
    w, o, _ = contig_words_np(contigs)
    need_n, need_w = len(contigs), len(w)
    off = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)
    bases = np.frombuffer("".join(contigs).encode(), np.uint8).copy()
    d_src, src_len = P.on_device(P.path_text(contigs))
    ops = {
        "rfx_dev_contigs_pack": lambda co: L.rfx_dev_contigs_pack(ctx, bases.ctypes.data, off.ctypes.data, len(contigs), C.byref(co)),
        "rfx_dev_contigs_from_text": lambda co: L.rfx_dev_contigs_from_text(ctx, d_src.data_ptr(), src_len, C.byref(co)),
    }
    for name, call in ops.items():
        exact = P.sentinel(need_n, need_w)
        co = exact._c()
        assert call(co) == OK and (int(co.n), int(co.need_n), int(co.need_words)) == (need_n, need_n, need_w), name
        exact._take(co)
        raw_equals_fast(exact, contigs, (name, "exact"))
        for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
            d = P.sentinel(cap_n, cap_w)
            co = d._c()
            co.need_n = co.need_words = -77
            assert call(co) == E_CAP, (name, cap_n, cap_w)
            assert (int(co.need_n), int(co.need_words)) == (need_n, need_w), name
            assert P.untouched(d), (name, cap_n, cap_w)
    pk = rfx.contigs_pack(contigs)
    text = P.text_of(as_t_fast(contigs), 32)
    need = len(text)
    kept = sum(1 for s in contigs if len(s) >= 32)
    for cap in (need, need - 1):
        d_text = torch.full((need + 16,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ln, nc = C.c_int64(-77), C.c_int64(-77)
        st = L.rfx_dev_contigs_to_text(ctx, C.byref(pk._c()), 32, d_text.data_ptr(), cap, C.addressof(ln), C.addressof(nc))
        assert (st, ln.value, nc.value) == (OK if cap >= need else E_CAP, need, kept), cap
        assert bool((d_text[cap:] == FILL).all()), cap
        same_text(bytes(d_text[:cap].cpu().numpy()).decode(), text[:cap], ("text cap", cap))


# ---- (b) the three rounds at scale ------------------------------------------------------------------------------------------------------------
GROUP_KINDS = ("rc copy", "rc left end", "fwd right end", "two rc ends", "two fwd ends and the rc middle", "short stranger", "empty", "alone")
HUB = (20_000, 120, 400, 150)                                      # bases, pieces, bases a piece, a piece every
LONG_PAIR = 150_000
SHARED = (420, (700, 800), (900, 1000))                            # R, and what lies around it in its two hosts
LONGER_PAIR = 6_200_000                                            # set 4: one list of more than 393,216 equal distances
ROUND_SETS = {1: dict(groups=1_100, seed=1605),
              2: dict(groups=2_200, seed=1606, hubs=1, long_pairs=1, shared=40),
              3: dict(groups=9_000, seed=1607, hubs=1, long_pairs=1, shared=40),
              4: dict(groups=1_100, seed=1609, long_pairs=1, long_bases=LONGER_PAIR)}
# what oracle.dedup_contigs gives on them (tests/test_dedup_scale_inputs.py holds the oracle to it): the contigs in, after each
# round, the candidate pairs of each round, the marker rows left over in the final set
EXPECT = {1: dict(n=2_475, rounds=[1_815, 1_471, 1_447], candidates=[961, 455, 24], leftover=73),
          2: dict(n=5_193, rounds=[3_755, 3_070, 3_014], candidates=[2_120, 909, 56], leftover=182),
          3: dict(n=20_493, rounds=[14_975, 12_128, 11_933], candidates=[8_056, 3_703, 195], leftover=601),
          4: dict(n=2_477, rounds=[1_811, 1_458, 1_435], candidates=[961, 446, 23], leftover=60),
          "skew": dict(n=2_110, rounds=[1_080, 51, 51], candidates=[2_058, 1_029, 0], leftover=0)}
MARKER_ROWS = {1: (319_772, 592_696), 2: (687_816, 1_264_795), 3: (2_663_152, 4_926_531), 4: (720_356, 993_586)}      # of round 1, of round 2 on the input
STEP0_ENTRIES = {1: 21_210, 2: 52_205, 3: 183_450, 4: 434_828}     # round 1's step-0 distance list holds at least these (counted on the plan)


def round_set(groups, seed, hubs=0, long_pairs=0, shared=0, long_bases=LONG_PAIR):
    """`groups` groups, each a random contig S of 600..999 bases and what GROUP_KINDS[i % 8] names (flanks of 1..66 new bases, end
    pieces of 500 resp. 450 bases), then the hubs (a contig of 20,000 bases and the reverse complements of 120 pieces of it), the long
    pairs (long_bases bases and their reverse complement) and the shared pieces (rc(R) for an R inside two unrelated contigs), shuffled
    -> (contigs, plan); plan: one (L, [(strand, a, b), ..]) for every long contig of L bases whose shorts cover S[a:b] -- what the
    conditions of tests/test_dedup_scale_inputs.py are counted on"""
    rng = np.random.default_rng(seed)
    out, plan = [], []
    for i in range(groups):
        L = int(rng.integers(600, 1000))
        S = rand_seq(rng, L)
        f1, f2 = 1 + i % 66, 1 + i % 37
        kind = GROUP_KINDS[i % len(GROUP_KINDS)]
        out.append(S)
        if kind == "rc copy":
            out.append(rc(S))
            plan.append((L, [("rc", 0, L)]))
        elif kind == "rc left end":
            out.append(rc(rand_seq(rng, f1) + S[:500]))
            plan.append((L, [("rc", 0, 500)]))
        elif kind == "fwd right end":
            out.append(S[L - 500:] + rand_seq(rng, f1))
            plan.append((L, [("fwd", L - 500, L)]))
        elif kind == "two rc ends":
            out += [rc(rand_seq(rng, f1) + S[:450]), rc(S[L - 450:] + rand_seq(rng, f2))]
            plan.append((L, [("rc", 0, 450), ("rc", L - 450, L)]))
        elif kind == "two fwd ends and the rc middle":
            out += [rand_seq(rng, f1) + S[:450], S[L - 450:] + rand_seq(rng, f2), rc(S[100:L - 100])]
            plan.append((L, [("fwd", 0, 450), ("fwd", L - 450, L), ("rc", 100, L - 100)]))
        elif kind == "short stranger":
            out.append(rand_seq(rng, i % 300))
        elif kind == "empty":
            out.append("")
    for _ in range(hubs):
        L, pieces, piece, every = HUB
        S = rand_seq(rng, L)
        out.append(S)
        out += [rc(S[every * j:every * j + piece]) for j in range(pieces)]
        plan.append((L, [("rc", every * j, every * j + piece) for j in range(pieces)]))
    for _ in range(long_pairs):
        S = rand_seq(rng, long_bases)
        out += [S, rc(S)]
        plan.append((long_bases, [("rc", 0, long_bases)]))
    for _ in range(shared):
        r, (a0, a1), (b0, b1) = SHARED
        R = rand_seq(rng, r)
        out += [rand_seq(rng, a0) + R + rand_seq(rng, a1), rand_seq(rng, b0) + R + rand_seq(rng, b1), rc(R)]
    return [out[i] for i in rng.permutation(len(out))], plan


def round_set_and_oracle(which):
    contigs, _ = round_set(**ROUND_SETS[which])
    return contigs, want(("rounds", which), lambda: O.dedup_contigs(contigs))


@pytest.mark.parametrize("which", sorted(ROUND_SETS))
def test_the_three_rounds_past_the_launch_thresholds_through_both_routes(rfx, which):
    """set 1: the marker sort of round 1 on the top-digit path, of round 2 on two MSD levels; set 2: more than 4,096 contigs,
    more than 1,024 merges in round 1's step 0, a hub of 120 steps, the long pair's one run of 10,000 equal distances among
    thousands of short lists; set 3: thousands of merges a step, 33 + 13 key bits; set 4: a pair of 6,200,000 bases whose one list
    of 413,000 equal distances takes the distance sort past 393,216 keys of 33 + 10 bits, one oversized bucket that finishes by the
    LSD passes, and the search of k_dd_vote four levels deep.  Marker rows are left over in all four.  The pack route and the
    from-text route give oracle.dedup_contigs' contigs, round counts and text"""
    contigs, w = round_set_and_oracle(which)
    assert len(contigs) == EXPECT[which]["n"]
    P.both_routes(rfx, contigs, 500, w["rounds"][2], w["text"], EXPECT[which]["rounds"], ("set", which))


def test_the_two_host_forms_on_set_2(rfx):
    """rfx_dedup_contigs and rfx_dedup_contig_text (which reports the surviving contigs, of any length): survivors, text, rounds"""
    contigs, w = round_set_and_oracle(2)
    rounds = EXPECT[2]["rounds"]
    surv, text, rn = rfx.dedup_contigs(contigs, 500)
    assert rn == rounds
    same_list(surv, w["rounds"][2], "rfx_dedup_contigs")
    same_text(text, w["text"], "rfx_dedup_contigs")
    text, nc, rn = rfx.dedup_contig_text(P.path_text(contigs, junk=False), 500)
    assert rn == rounds and nc == len(w["rounds"][2])
    same_text(text, w["text"], "rfx_dedup_contig_text")


def test_set_2_into_exactly_the_reported_needs_and_one_short(rfx):
    """rfx_dev_dedup_contigs by hand, with marker rows left over: the needs it reports are the oracle's contigs and their words; a
    set of exactly that size takes the oracle's contigs; one contig or one word short is RFX_E_CAP with the needs and nothing written"""
    contigs, w = round_set_and_oracle(2)
    final = w["rounds"][2]
    pk = rfx.contigs_pack(contigs)
    ci = pk._c()
    rn = (C.c_int64 * 3)()

    def call(co):
        return rfx.L.rfx_dev_dedup_contigs(rfx.ctx, C.byref(ci), C.byref(co), C.addressof(rn))
    need_n, need_w = len(final), sum((len(s) + 31) // 32 for s in final)
    probe = P.sentinel(0, 0)
    co = probe._c()
    assert call(co) == E_CAP and (int(co.need_n), int(co.need_words)) == (need_n, need_w) and P.untouched(probe)
    exact = P.sentinel(need_n, need_w)
    co = exact._c()
    assert call(co) == OK and int(co.n) == need_n and [int(x) for x in rn] == [len(r) for r in w["rounds"]]
    exact._take(co)
    same_list(rfx.contigs_unpack(exact), final, "exact")
    raw_equals_fast(exact, final, "exact")
    for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
        d = P.sentinel(cap_n, cap_w)
        co = d._c()
        co.need_n = co.need_words = -77
        assert call(co) == E_CAP, (cap_n, cap_w)
        assert (int(co.need_n), int(co.need_words)) == (need_n, need_w) and P.untouched(d), (cap_n, cap_w)


# ---- (c) skew ---------------------------------------------------------------------------------------------------------------------------------
SKEW = (1_030, 700, 50, 800)                                       # copies of S and of rc(S), bases of S, strangers, their bases
SKEW_SEED = 1608


def skew_set():
    """1,030 copies of one contig of 700 bases, 1,030 of its reverse complement and 50 unrelated contigs of 800 bases, shuffled
    -> (contigs, S)"""
    copies, L, strangers, Ls = SKEW
    rng = np.random.default_rng(SKEW_SEED)
    S = rand_seq(rng, L)
    out = [S] * copies + [rc(S)] * copies + [rand_seq(rng, Ls) for _ in range(strangers)]
    return [out[i] for i in rng.permutation(len(out))], S


def test_two_thousand_copies_of_one_contig(rfx):
    """every seed 31-mer under a probe window is a run of 2,060 equal keys (more than a sort tile, more than eight blocks of
    k_dd_select; top-digit buckets that finish by the LSD passes), and one group of more than a thousand shorts makes a round of more
    than a thousand steps of one merge each.  The time of the call is printed (DESIGN.md section 20 records it)"""
    contigs, _ = skew_set()
    w = want(("skew",), lambda: O.dedup_contigs(contigs))
    rounds = EXPECT["skew"]["rounds"]
    pk = rfx.contigs_pack(contigs)
    t0 = time.perf_counter()
    out, rn = rfx.dedup_dev(pk)
    print(f"\nskewed set: rfx_dev_dedup_contigs took {time.perf_counter() - t0:.3f} s, rounds {rn}")
    assert rn == rounds
    same_list(rfx.contigs_unpack(out), w["rounds"][2], "skew")
    raw_equals_fast(out, w["rounds"][2], "skew")
    same_text(P.device_text(rfx, out, 500)[0], w["text"], "skew")
    d_text, ln = P.on_device(P.path_text(contigs, junk=False))
    out2, rn2 = rfx.dedup_dev(rfx.contigs_from_text_dev(d_text, ln))
    assert rn2 == rounds
    raw_equals_fast(out2, w["rounds"][2], "skew, text route")


# ---- (d) poisoned allocations -----------------------------------------------------------------------------------------------------------------
def test_everything_again_with_every_allocation_poisoned(tmp_path):
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is 0xA5 before the library uses it.  A child process (the mask is read
    once per process), which takes the oracle's results from a file this process writes"""
    for which in ROUND_SETS:
        round_set_and_oracle(which)
    want(("skew",), lambda: O.dedup_contigs(skew_set()[0]))
    path = tmp_path / "want.pickle"
    with open(path, "wb") as f:
        pickle.dump(_want, f)
    env = dict(os.environ, RFX_POISON="7", **{WANT_ENV: str(path)})
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
