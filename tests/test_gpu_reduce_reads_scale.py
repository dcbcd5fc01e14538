"""The entry points of DESIGN.md section 32 past the sizes where their launches change shape (section 20): the sorter from the counter's
arrays (rfx_dev_ksort_from_counts, rfx_dev_ksort_run_counts), the packed union and reduction (rfx_dev_reduce_union_packed,
rfx_dev_reduce_run_packed), rfx_dev_dyn_from_kmers, and the driver in both forms (rfx_dev_reduce_reads, rfx_reduce_reads).  Their own
files stay inside one look-back scan tile, where the scan of the keep flags is nearly the identity; here every input has dropped rows or
records of a foreign length all over it, at 4,096 / 4,097 / 8,193 rows, above 262,144 and above 65,536 union rows.

Every comparison is exact and against a model, never against another entry point: the string models (ksort_model binarize /
run_stages / handover, reduce_model union / run_stages / handover, reduce_reads_model.model) or a numpy statement of one of them that
tests/test_reduce_reads_scale_inputs.py pins to it on the CPU, where the conditions on the inputs are asserted too.  Sets are compared
with equals_fast of tests/test_gpu_dynamic_scale.py: field by field after unpack and word for word against the numpy packer."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import ksort_model as K
from tests import reduce_model as R
from tests import reduce_reads_model as RR
from tests import test_gpu_dynamic_scale as S
from tests import test_gpu_ksort as TK
from tests.test_gpu_dynamic_scale import ksort_rows, reduce_model_run, dyn_records, equals_fast, host_kmer      # (equals_fast: np_packed_fast)
from tests.test_gpu_dynamic_scale import REDUCE_K, REDUCE_P
from tests.test_gpu_ksort_counts import on_device, MAX_COV
from tests.test_gpu_map import dev_reads
from tests.test_gpu_reduce_reads_model import first_difference

pytestmark = pytest.mark.gpu

NUC = np.frombuffer(b"ACGT", np.uint8)
CODE = np.zeros(256, np.uint8)
CODE[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
TILE = 4096                                                         # rfx_scan.hip: LB_TILE
CLAMP = 30000


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


# ---- what the string models give, made once: in this process, or by the parent of the poisoned run -----------------------------------------
WANT_ENV = "RFX_SCALE_WANT"                                        # a pickle of {key: value} the parent process wrote
_want = {}


def want(key, make):
    if not _want and os.environ.get(WANT_ENV):
        with open(os.environ[WANT_ENV], "rb") as f:
            _want.update(pickle.load(f))
    if key not in _want:
        _want[key] = make()
    return _want[key]


def ksort_want(k):
    """ksort_rows(k) through the cached model run -> (stage s8 as a record set, its text)"""
    def make():
        st = S.ksort_model_run(k)["st"]
        return host_kmer(st["s8"]), K.to_text(st["s8"], k)
    return want(("ksort", k), make)


def reduce_want():
    """the cached reduce_model.run_stages -> {union, neutral: record sets; text: both final texts}"""
    def make():
        st = reduce_model_run()["st"]
        return dict(union=host_kmer(st["union"]), neutral=host_kmer(st["neutral"]), text=[R.to_text(st["neutral"], k) for k in REDUCE_K])
    return want(("reduce",), make)


def driver_want():
    """reduce_reads_model.model on the driver's read set -> the text of every Count_<k>_reduced"""
    return want(("driver",), lambda: RR.model(scale_reads(), SCALE_KLIST, P=SCALE_P))


WANT_MAKERS = (lambda: ksort_want(31), lambda: ksort_want(95), reduce_want, driver_want)


# ---- k-mers as code arrays ----------------------------------------------------------------------------------------------------------------
def kmer_strings(codes):
    """[n, k] base codes -> n strings"""
    n, k = codes.shape
    text = NUC[codes.reshape(-1)].tobytes().decode()
    return [text[i * k:(i + 1) * k] for i in range(n)]


def kmer_codes(kmers, k):
    return CODE[np.frombuffer("".join(kmers).encode(), np.uint8)].reshape(len(kmers), k)


def counter_words_np(codes, k, rng=None):
    """counter_words of tests/test_gpu_ksort_counts.py without a loop over the rows: k // 32 full words of 32 bases, the first in the
    highest bits, then the k % 32 last bases right-aligned in one word; rng: junk above the bases of that last word"""
    n, W = len(codes), k // 32 + 1
    out = np.zeros((n, W), np.uint64)
    for j in range(W):
        part = codes[:, 32 * j:32 * j + 32].astype(np.uint64)
        m = part.shape[1]
        if m:
            out[:, j] = np.bitwise_or.reduce(part << (np.uint64(2) * (np.uint64(m - 1) - np.arange(m, dtype=np.uint64))), axis=1)
        if rng is not None and j == W - 1 and 0 < m < 32:
            out[:, j] |= rng.integers(0, 1 << 20, n).astype(np.uint64) << np.uint64(2 * m)
    return out


# ---- a. the sorter from the counter's arrays ------------------------------------------------------------------------------------------------
# (solid rows, extra rows): 4,096, 4,097 and 8,193 rows with the seam between the two arrays inside the first tile, and 12,290 rows
# with the seam in the third, so that three tiles of solid rows hold dropped rows (an extra row's count is 1: it cannot be dropped)
COUNT_CASES = ((4000, 96), (4000, 97), (4000, 4193), (12_000, 290))
COUNT_KS = (31, 65)                                                # one word and int32 counts; three words and int64 counts
COUNT_LARGE = (260_000, 10_000, 41)                                # 66 tiles
KEPT_COUNTS = np.array([1, 8, CLAMP - 1, CLAMP, CLAMP + 1, MAX_COV])
DROPPED_COUNTS = np.array([MAX_COV + 1, 999_999_999])
DROP_ONE_IN = 64


def counts_input(n, n_extra, k):
    """n solid rows and n_extra extra rows of random k-mers -> (codes [n + n_extra, k], the solid rows' counts); a solid row's count is
    above max_cov with probability 1 / 64, drawn row by row"""
    rng = np.random.default_rng(1000 * k + n + n_extra)
    codes = rng.integers(0, 4, (n + n_extra, k), dtype=np.uint8)
    drop = rng.random(n) < 1.0 / DROP_ONE_IN
    return codes, np.where(drop, rng.choice(DROPPED_COUNTS, n), rng.choice(KEPT_COUNTS, n)).astype(np.int64)


def count_rows(codes, counts):
    """the `KMER,count` rows a printer makes of the two arrays: the solid rows, then the extra rows with count 1"""
    s, n = kmer_strings(codes), len(counts)
    return [f"{a},{int(c)}\n" for a, c in zip(s[:n], counts)] + [f"{a},1\n" for a in s[n:]]


def binarize_np(codes, counts, k, max_cov=MAX_COV):
    """ksort_model.binarize on count_rows(codes, counts): a count of ten digits or more reads as 1,000,000,000, a row above max_cov is
    dropped, a kept row gives its k-mer's record and then its reverse complement's with left = right = the count clamped to 30000"""
    c = np.concatenate([counts, np.ones(len(codes) - len(counts), np.int64)])
    c = np.minimum(c, 1_000_000_000)
    keep = c <= max_cov
    f = codes[keep]
    both = np.stack([f, (3 - f)[:, ::-1]], axis=1).reshape(-1, k)
    m = len(both)
    cl = np.repeat(np.minimum(c[keep], CLAMP), 2)
    return dyn_records(both[:, :k - 1].reshape(-1), np.arange(m + 1) * (k - 1), both[:, k - 1], np.arange(m + 1), np.ones(m), cl, cl)


def counts_on_device(codes, counts, k):
    """-> (keys, counts, extra keys) in HBM in the counter's format, junk above the last word's bases, int32 counts at k <= 31"""
    n = len(counts)
    words = counter_words_np(codes, k, np.random.default_rng(k))
    dk, dc = on_device(words[:n], counts, np.int32 if k <= 31 else np.int64)
    dx, _ = on_device(words[n:]) if len(codes) > n else (None, None)
    return dk, dc, dx


@pytest.mark.parametrize("k", COUNT_KS, ids=lambda k: f"k{k}")
@pytest.mark.parametrize("n,n_extra", COUNT_CASES)
def test_from_counts_with_dropped_rows_in_one_two_and_three_scan_tiles(rfx, n, n_extra, k):
    """k_kc_keep, the look-back scan of its flags and k_kc_emit's 2 s + h: ksort_model.binarize on the printed rows"""
    codes, counts = counts_input(n, n_extra, k)
    dk, dc, dx = counts_on_device(codes, counts, k)
    got = rfx.ksort_from_counts(dk, dc, rfx.ksort_params(k), d_extra=dx)
    recs = K.binarize(count_rows(codes, counts), K.default_params(k))
    assert got.n == len(recs) == 2 * (int((counts <= MAX_COV).sum()) + n_extra) < 2 * (n + n_extra)
    equals_fast(rfx, got, host_kmer(recs), ("from_counts", n, n_extra, k))


def test_from_counts_on_270000_rows(rfx):
    """66 tiles, so a tile has more predecessors than one lane window of the look-back covers; the numpy statement of binarize"""
    n, n_extra, k = COUNT_LARGE
    codes, counts = counts_input(n, n_extra, k)
    dk, dc, dx = counts_on_device(codes, counts, k)
    got = rfx.ksort_from_counts(dk, dc, rfx.ksort_params(k), d_extra=dx)
    equals_fast(rfx, got, binarize_np(codes, counts, k), ("from_counts", n, n_extra, k))


@pytest.mark.parametrize("k", [31, 95])
def test_run_counts_on_70000_rows(rfx, k):
    """steps 1-8 from the arrays on the rows of test_ksort_chain_on_70000_rows: stage s8 of the same model run, and its text"""
    rows = ksort_rows(k)
    kmers, counts = zip(*(r.rstrip("\n").split(",") for r in rows))
    codes, counts = kmer_codes(kmers, k), np.array(counts, np.int64)
    dk, dc, _ = counts_on_device(codes, counts, k)
    s8, text = ksort_want(k)
    out = rfx.ksort_run_counts(dk, dc, TK.cparams(rfx, K.default_params(k)))
    equals_fast(rfx, out, s8, ("run_counts", k))
    assert TK.text_of(rfx, out, k) == text


# ---- b. the packed union and the packed reduction -------------------------------------------------------------------------------------------
FOREIGN_LEN, FOREIGN_ONE_IN = 36, 40
UNION_CUTS = (4096, 4097)
LARGE_LONG, LARGE_SHORT = 270_000, 9000
_inputs = {}


def kmer_set_np(rng, lengths):
    """full k-mers of the given lengths as a record set: random bases, no extension, marker 1, left and right over the whole range the
    text keeps, its two ends included"""
    n = len(lengths)
    off = S.offsets_of(np.asarray(lengths, np.int64))
    lr = lambda: np.where(rng.random(n) < 0.05, rng.choice([-CLAMP, CLAMP], n), rng.integers(-CLAMP, CLAMP + 1, n))   # noqa: E731
    return dyn_records(rng.integers(0, 4, off[-1], dtype=np.uint8), off, np.zeros(0, np.uint8), np.zeros(n + 1, np.int64), np.ones(n), lr(), lr())


def with_foreign(own, seed):
    """own's records in their order, and one record in 40 of FOREIGN_LEN bases among them at positions drawn from the generator"""
    rng = np.random.default_rng(seed)
    m = own.n // (FOREIGN_ONE_IN - 1) + 8
    at = np.zeros(own.n + m, bool)
    at[rng.choice(own.n + m, m, replace=False)] = True
    idx = np.empty(own.n + m, np.int64)
    idx[at], idx[~at] = own.n + np.arange(m), np.arange(own.n)
    return S.take(S.concat(own, kmer_set_np(rng, np.full(m, FOREIGN_LEN))), idx)


def key_lengths(r):
    return np.diff(r.key_off[:r.n + 1])


def packed_inputs():
    """the two row lists of reduce_model_run() as sets of full k-mers with foreign records among them -> (short, long), and the large
    union's numpy-made sets: a long one of 270,000 records of k2 and k1 bases, a short one of 9,000 of k1, k2 and foreign bases"""
    if not _inputs:
        k1, k2 = REDUCE_K
        rs, rl = S.reduce_rows()
        _inputs["short"] = with_foreign(host_kmer(R.parse_rows(rs, REDUCE_K)), 1)
        _inputs["long"] = with_foreign(host_kmer(R.parse_rows(rl, REDUCE_K)), 2)
        rng = np.random.default_rng(270)
        _inputs["large_long"] = kmer_set_np(rng, rng.choice([k2, k2, k2, k1], LARGE_LONG))
        _inputs["large_short"] = kmer_set_np(rng, rng.choice([k1, k1, k2, FOREIGN_LEN], LARGE_SHORT))
    return _inputs


def select_np(r, length):
    """the records of r whose key has `length` bases, left and right clamped as the text clamps them"""
    t = S.take(r, np.flatnonzero(key_lengths(r) == length))
    t.left[:], t.right[:] = np.clip(t.left, -CLAMP, CLAMP), np.clip(t.right, -CLAMP, CLAMP)
    return t


def union_np(short, long, k1, k2):
    """reduce_model.union on the texts of the two sets (to_text(short, k1), to_text(long, k2)): the long set's records of k2 bases, then
    the short set's of k1 bases"""
    return S.concat(select_np(long, k2), select_np(short, k1))


def handover_np(r, k):
    """the handover models on to_text(r, k): the records of k bases as (the first k - 1 bases, the last base, 1, left, right)"""
    t = select_np(r, k)
    codes = t.key[:t.n * k].reshape(t.n, k)
    return dyn_records(codes[:, :k - 1].reshape(-1), np.arange(t.n + 1) * (k - 1), codes[:, k - 1], np.arange(t.n + 1), np.ones(t.n), t.left, t.right)


def concat_all(sets):
    out = sets[0]
    for s in sets[1:]:
        out = S.concat(out, s)
    return out


@pytest.fixture(scope="module")
def packed(rfx):
    """-> {name: (record set, packed set in HBM)}"""
    return {name: (r, rfx.dyn_pack(r)) for name, r in packed_inputs().items()}


def test_union_packed_drops_foreign_records_in_every_tile(rfx, packed):
    """ks_select_length's flags with zeros everywhere, their scans over 7 and 27 tiles, k_rd_pk_emit by rank and with its base: stage
    `union` of the cached model run"""
    (short, d_short), (long, d_long) = packed["short"], packed["long"]
    want_u = reduce_want()["union"]
    got = rfx.reduce_union_packed(d_short, d_long, rfx.reduce_params(*REDUCE_K))
    assert got.n == want_u.n < short.n + long.n
    equals_fast(rfx, got, want_u, "union")


@pytest.mark.parametrize("cut", UNION_CUTS)
def test_union_packed_with_the_short_set_cut_at_a_tile_edge(rfx, packed, cut):
    """the short set's first 4,096 and 4,097 records, the foreign ones counted: one tile and one record into the second"""
    (short, _), (_, d_long) = packed["short"], packed["long"]
    k1, k2 = REDUCE_K
    head = S.take(short, np.arange(cut))
    own = int((key_lengths(head) == k1).sum())
    rs, rl = S.reduce_rows()
    recs = R.union(rs[:own], rl, k1, k2)
    got = rfx.reduce_union_packed(rfx.dyn_pack(head), d_long, rfx.reduce_params(k1, k2))
    assert got.n == len(recs) and 0 < own < cut
    equals_fast(rfx, got, host_kmer(recs), ("union", cut))


def test_run_packed_on_the_full_set(rfx, packed):
    """the whole reduction from the two packed sets: stage `neutral` at REDUCE_P and both texts"""
    w = reduce_want()
    out = rfx.reduce_run_packed(packed["short"][1], packed["long"][1], REDUCE_P, rfx.reduce_params(*REDUCE_K))
    equals_fast(rfx, out, w["neutral"], "run_packed")
    for k, text in zip(REDUCE_K, w["text"]):
        got = TK.text_of(rfx, out, k)
        assert got == text, ("text", k, first_difference(got, text))


def test_union_packed_with_a_long_set_of_270000_records(rfx, packed):
    """66 tiles of flags for the long set, a quarter of them 0; the short set holds records of the long length and of a foreign one"""
    (short, d_short), (long, d_long) = packed["large_short"], packed["large_long"]
    got = rfx.reduce_union_packed(d_short, d_long, rfx.reduce_params(*REDUCE_K))
    equals_fast(rfx, got, union_np(short, long, *REDUCE_K), "large union")


# ---- c. full k-mers -> the sub-k-mer records of the dynamic-k passes ------------------------------------------------------------------------
FROM_KMERS_LISTS = ((31, 41), (41, 31), (41,))


@pytest.fixture(scope="module")
def neutral(rfx):
    r = reduce_want()["neutral"]
    return r, rfx.dyn_pack(r)


@pytest.mark.parametrize("lens", FROM_KMERS_LISTS, ids=lambda l: "_".join(map(str, l)))
def test_dyn_from_kmers_on_the_reduced_set(rfx, neutral, lens):
    """113,413 records of two lengths (stage `neutral` of the model run, packed here), one set with a list of lengths: the handover form length by length"""
    r, d = neutral
    got = rfx.dyn_from_kmers([d] * len(lens), lens)
    equals_fast(rfx, got, concat_all([handover_np(r, k) for k in lens]), ("from_kmers", lens))


def test_dyn_from_kmers_on_three_sets_with_an_empty_one_between(rfx, neutral, packed):
    """k_ks_kmer_emit's base behind 22 tiles and behind an empty set, then 66 tiles of flags with zeros"""
    k1, k2 = REDUCE_K
    (r, d), (big, d_big) = neutral, packed["large_long"]
    empty = rfx.dyn_pack(host_kmer([]))
    got = rfx.dyn_from_kmers([d, empty, d_big], [k1, k2, k2])
    equals_fast(rfx, got, S.concat(handover_np(r, k1), handover_np(big, k2)), "three sets")


# ---- d. the driver ------------------------------------------------------------------------------------------------------------------------
SCALE_SEED, SCALE_G, SCALE_KLIST, SCALE_P = 32, 23_000, (23, 41, 67), 3
SCALE_READ = (100, 150)
SCALE_DEPTHS = (10, 4)
DEV_FIRST_CAP = 4096                                               # the records the caller's set holds at the first call


def scale_reads(G=SCALE_G):
    """a random genome of G bases; reads of 100..150 bases at depth 10 from it and at depth 4 from a copy with one changed base about
    every 300; behind them the planted fork of reduce_reads_model.forked_reads with its three extra reads cut to 150 bases (12 x s,
    7 x v, 3 x random(18) + v[36:] + random(18)), without which no later k's E reaches a text: at depth 4 the minor allele of a
    changed base is an error at every k under E = 6 and under E = 8 alike"""
    rng = np.random.default_rng(SCALE_SEED)
    g = rng.integers(0, 4, G, dtype=np.uint8)
    v = g.copy()
    at = np.arange(150, G - 40, 300)
    at = at + rng.integers(-40, 40, len(at))
    v[at] = (v[at] + rng.integers(1, 4, len(at))) % 4
    reads = []
    for src, depth in zip((g, v), SCALE_DEPTHS):
        text = NUC[src].tobytes().decode()
        total = 0
        while total < depth * G:
            n = int(rng.integers(SCALE_READ[0], SCALE_READ[1] + 1))
            p = int(rng.integers(0, G - n + 1))
            reads.append(text[p:p + n])
            total += n
    s = RR.rnd(rng, 150)
    f = s[:100] + "ACGT"[("ACGT".index(s[100]) + 2) % 4] + s[101:]
    return reads + [s] * 12 + [f] * 7 + [RR.rnd(rng, 18) + f[RR.FORK_TAIL:] + RR.rnd(rng, 18) for _ in range(3)]


@pytest.fixture(scope="module")
def driver():
    """-> (the reads, the model's text of every Count_<k>_reduced): the one fixture that pays for reduce_reads_model.model"""
    return scale_reads(), driver_want()


def test_reduce_reads_text_equals_the_model(rfx, driver):
    """rfx_reduce_reads: counter rows above the first capacity at every k, unions above 65,793 rows, a pair's final set as the next
    pair's short input, E = 6 at k = 67 -- byte for byte"""
    reads, texts = driver
    got = rfx.reduce_reads_text([r.encode() for r in reads], SCALE_KLIST, rfx.reduce_reads_params(P=SCALE_P))
    for k, g, w in zip(SCALE_KLIST, got, texts):
        g = g.decode()
        assert g == w, (f"Count_{k}_reduced", first_difference(g, w))


def test_reduce_reads_dev_equals_the_model(rfx, driver):
    """rfx_dev_reduce_reads on the 2-bit read store: out_n_per_k and the set, which is the handover form of the model's texts in list
    order; the caller's set has room for 4,096 records, so the whole call runs once more at the size it reports"""
    from reflexiv_amd.api import DynPacked
    reads, texts = driver
    dw, dn, wpr = dev_reads(reads)
    dev, per_k = rfx.reduce_reads_dev(dw, dn, len(reads), wpr, max(len(r) for r in reads), SCALE_KLIST, rfx.reduce_reads_params(P=SCALE_P),
                                      out=DynPacked(DEV_FIRST_CAP, DEV_FIRST_CAP))
    assert per_k == [t.count("\n") for t in texts] and sum(per_k) > DEV_FIRST_CAP
    equals_fast(rfx, dev, host_kmer([rec for t in texts for rec in R.handover(t)]), "reduce_reads_dev")


# ---- e. poisoned allocations ----------------------------------------------------------------------------------------------------------------
def test_everything_again_with_every_allocation_poisoned(tmp_path):
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is 0xA5 before the library uses it.  A child process (the mask is read
    once per process), which takes what the string models gave from a file this process writes"""
    for make in WANT_MAKERS:
        make()
    path = tmp_path / "want.pickle"
    with open(path, "wb") as f:
        pickle.dump(_want, f)
    env = dict(os.environ, RFX_POISON="7", **{WANT_ENV: str(path)})
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
