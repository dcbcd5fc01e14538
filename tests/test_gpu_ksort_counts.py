"""The k-mer sorting stage straight from the counter's arrays (rfx_dev_ksort_from_counts, rfx_dev_ksort_run_counts; DESIGN.md section
32).  The expected set is always what the text path gives -- rfx_dev_ksort_binarize / rfx_dev_ksort_run on the `KMER,count` rows a
Python helper prints from the same arrays -- and the two sets are compared array by array, whole words: keys with their padding
bits and unused words, extensions, offsets, lengths, markers, left and right.  Random keys, no reads."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_gpu_dynamic_packed import poisoned, untouched, OK, E_ARG, E_CAP
from tests.test_gpu_ksort import upload

pytestmark = pytest.mark.gpu

KS = (8, 23, 31, 33, 34, 62, 65, 66, 95, 97, 124)
NS = (0, 1, 255, 256, 257, 1000)
MAX_COV = 10_000_000
COUNTS = (1, 8, 30000, 30001, MAX_COV, MAX_COV + 1, 999_999_999)
NUC = "ACGT"
COMP = str.maketrans("ACGT", "TGCA")
FIELDS = ("key", "key_len", "ext", "ext_off", "ext_len", "marker", "left", "right")


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


def kmers_of(rng, k, n):
    """n distinct k-mers, ascending: random ones, pairs that fork (the same k - 1 first bases, the same k - 1 last bases), all A, all
    T and one that is its own reverse complement (even k)"""
    out = set()
    if n >= 3:
        out |= {"A" * k, "T" * k}
        half = "".join(NUC[b] for b in rng.integers(0, 4, k // 2))
        if k % 2 == 0:
            out.add(half + half[::-1].translate(COMP))
    while len(out) < n:
        s = "".join(NUC[b] for b in rng.integers(0, 4, k))
        out.add(s)
        if len(out) < n and rng.integers(0, 8) == 0:
            out.add(s[:-1] + NUC[(NUC.index(s[-1]) + 1 + int(rng.integers(0, 3))) % 4])
        if len(out) < n and rng.integers(0, 8) == 0:
            out.add(NUC[(NUC.index(s[0]) + 1 + int(rng.integers(0, 3))) % 4] + s[1:])
    return sorted(out)


def counter_words(kmers, k, rng=None):
    """the counter's key format: k // 32 full words of 32 bases, then the k % 32 last bases in the lowest bits of one word (k <= 31:
    that word alone); rng: junk above the bases of the last word, which the entry points must ignore"""
    W = k // 32 + 1
    out = np.zeros((len(kmers), W), np.uint64)
    for i, s in enumerate(kmers):
        for j in range(W):
            part = s[32 * j:32 * j + 32]
            v = 0
            for ch in part:
                v = (v << 2) | NUC.index(ch)
            if rng is not None and j == W - 1 and 0 < len(part) < 32:
                v |= int(rng.integers(0, 1 << 20)) << (2 * len(part)) & 0xFFFFFFFFFFFFFFFF
            out[i, j] = v
    return out


def on_device(keys, counts=None, dtype=None):
    import torch
    dk = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64).reshape(-1).copy()).cuda()
    dc = torch.from_numpy(np.asarray(counts, dtype).copy()).cuda() if counts is not None else None
    torch.cuda.synchronize()
    return dk, dc


def rows_of(kmers, counts, extra):
    return [f"{s},{int(c)}\n" for s, c in zip(kmers, counts)] + [f"{s},1\n" for s in extra]


def same_set(got, want, tag):
    assert got.n == want.n, (tag, got.n, want.n)
    for name, a, b in zip(FIELDS, got.host(), want.host()):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (tag, name)


def extras_of(rng, kmers, k, m):
    """m extra keys with duplicates: some of the solid k-mers, some new ones, some twice"""
    if m == 0:
        return []
    pool = list(kmers[:5]) + ["".join(NUC[b] for b in rng.integers(0, 4, k)) for _ in range(max(1, m // 2))]
    return [pool[int(rng.integers(0, len(pool)))] for _ in range(m)]


@pytest.mark.parametrize("n", NS, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("k", KS, ids=lambda k: f"k{k}")
def test_both_entry_points_equal_the_text_path_on_the_printed_rows(rfx, k, n):
    """every k of the list (one word; W = 2, 3, 4 with residues 1, 2, 30, 31; sub-k-mers on both sides of 32, 64 and 96) x every n
    (around the block size) x 0, 1 and 300 extra rows x (E, bubble) in (8, 1), (6, 1), (8, 0); the counts cycle through the clamp at
    30000, max_cov, max_cov + 1 and nine digits; int32 counts at k <= 31 and int64 above, as the counters write them"""
    rng = np.random.default_rng(1000 * k + n)
    kmers = kmers_of(rng, k, n)
    counts = [COUNTS[int(i)] for i in rng.permutation(len(kmers)) % len(COUNTS)]
    dtype = np.int32 if k <= 31 else np.int64
    dk, dc = on_device(counter_words(kmers, k, rng), counts, dtype)
    for m in (0, 1, 300):
        extra = extras_of(rng, kmers, k, m)
        dx, _ = on_device(counter_words(extra, k))
        text = upload(rows_of(kmers, counts, extra))
        cp = rfx.ksort_params(k, max_k=max(95, k))
        got = rfx.ksort_from_counts(dk, dc, cp, d_extra=dx if m else None)
        want = rfx.ksort_binarize(*text, cp)
        same_set(got, want, (k, n, m, "from_counts"))
        kept = sum(c <= MAX_COV for c in counts) + m
        assert got.n == 2 * kept
        for E, bubble in ((8, 1), (6, 1), (8, 0)):
            cp = rfx.ksort_params(k, max_k=max(95, k), min_error_cov=E, bubble=bubble)
            same_set(rfx.ksort_run_counts(dk, dc, cp, d_extra=dx if m else None), rfx.ksort_run(*text, cp), (k, n, m, E, bubble, "run_counts"))


@pytest.mark.parametrize("k", [23, 65])
def test_counts_of_ten_digits_behave_as_1_000_000_000(rfx, k):
    """max_cov = 2^31 - 1: 1,000,000,000 and 2^31 - 1 (both widths) and 2^40 (int64) are kept, as the text rule for ten digits or more
    keeps them, and clamp to 30000; with the default max_cov the same rows are dropped"""
    rng = np.random.default_rng(k)
    kmers = kmers_of(rng, k, 40)
    for dtype, big in ((np.int32, (1_000_000_000, 2**31 - 1)), (np.int64, (1_000_000_000, 2**31 - 1, 2**40, 2**62))):
        counts = [(big + (3, 999_999_999, 30000))[i % (len(big) + 3)] for i in range(len(kmers))]
        dk, dc = on_device(counter_words(kmers, k), counts, dtype)
        text = upload(rows_of(kmers, counts, []))
        for max_cov in (2**31 - 1, 1_000_000_000, 999_999_999, MAX_COV):
            cp = rfx.ksort_params(k, max_cov=max_cov)
            got = rfx.ksort_from_counts(dk, dc, cp)
            same_set(got, rfx.ksort_binarize(*text, cp), (k, dtype, max_cov))
            same_set(rfx.ksort_run_counts(dk, dc, cp), rfx.ksort_run(*text, cp), (k, dtype, max_cov, "run"))
            kept = sum(min(c, 1_000_000_000) <= max_cov for c in counts)
            assert got.n == 2 * kept and (max_cov < 1_000_000_000 or kept == len(kmers))
            if max_cov == 2**31 - 1:
                assert sorted(set(got.left[:got.n].cpu().tolist())) == [3, 30000]


def test_the_other_count_width_and_extra_rows_alone(rfx):
    """count_bytes is the caller's: int64 counts at k <= 31 and int32 counts at k > 31; no solid rows at all; max_cov = 0 drops the
    extra rows (1 > 0) as the text path drops `KMER,1`"""
    rng = np.random.default_rng(7)
    for k, dtype in ((31, np.int64), (33, np.int32)):
        kmers = kmers_of(rng, k, 300)
        counts = [COUNTS[i % len(COUNTS)] for i in range(len(kmers))]
        dk, dc = on_device(counter_words(kmers, k), counts, dtype)
        extra = extras_of(rng, kmers, k, 17)
        dx, _ = on_device(counter_words(extra, k))
        cp = rfx.ksort_params(k)
        same_set(rfx.ksort_from_counts(dk, dc, cp, d_extra=dx), rfx.ksort_binarize(*upload(rows_of(kmers, counts, extra)), cp), (k, "width"))
        same_set(rfx.ksort_run_counts(None, None, cp, n=0, d_extra=dx), rfx.ksort_run(*upload(rows_of([], [], extra)), cp), (k, "extra alone"))
        cp0 = rfx.ksort_params(k, max_cov=0)
        dz, dc0 = on_device(counter_words(kmers[:3], k), [0, 1, 0], dtype)
        got = rfx.ksort_from_counts(dz, dc0, cp0, d_extra=dx)
        same_set(got, rfx.ksort_binarize(*upload(rows_of(kmers[:3], [0, 1, 0], extra)), cp0), (k, "max_cov 0"))
        assert got.n == 4


def test_an_empty_input(rfx):
    for k in (31, 65):
        cp = rfx.ksort_params(k)
        for fn in (rfx.ksort_from_counts, rfx.ksort_run_counts):
            out = fn(None, None, cp, n=0)
            assert out.n == 0 and int(out.ext_off[0]) == 0


def call(rfx, fn, dk, dc, nbytes, n, dx, nx, cp, co):
    return fn(rfx.ctx, dk.data_ptr() if dk is not None else None, dc.data_ptr() if dc is not None else None, nbytes, n,
              dx.data_ptr() if dx is not None else None, nx, C.byref(cp) if cp is not None else None, C.byref(co) if co is not None else None)


def test_refused_arguments_write_nothing(rfx):
    """a k the sorter refuses (32, 63, 94, 7, 125), a k the counter does not write (64, 96), a negative count in either width,
    count_bytes other than 4 or 8, negative n, null pointers, the sorter's own parameter checks"""
    rng = np.random.default_rng(3)
    k = 33
    kmers = kmers_of(rng, k, 50)
    dk, dc = on_device(counter_words(kmers, k), [5] * 50, np.int64)
    dx, _ = on_device(counter_words(kmers[:4], k))
    good = rfx.ksort_params(k)
    for fn in (rfx.L.rfx_dev_ksort_from_counts, rfx.L.rfx_dev_ksort_run_counts):
        d = poisoned(200, 200)

        def refused(*a):
            co = d._c()
            co.n = co.need_words = -77
            st = call(rfx, fn, *a, co)
            return st == E_ARG and untouched(d) and (int(co.n), int(co.need_words)) == (-77, -77)

        assert call(rfx, fn, dk, dc, 8, 50, dx, 4, good, d._c()) == OK and not untouched(d)
        d = poisoned(200, 200)
        for bad_k in (32, 63, 94, 7, 125, 64, 96):
            assert refused(dk, dc, 8, 50, dx, 4, rfx.ksort_params(bad_k)), bad_k
        for nbytes in (0, 2, 16, -4):
            assert refused(dk, dc, nbytes, 50, dx, 4, good), nbytes
        assert refused(dk, dc, 8, -1, dx, 4, good) and refused(dk, dc, 8, 50, dx, -1, good)
        assert refused(None, dc, 8, 50, dx, 4, good) and refused(dk, None, 8, 50, dx, 4, good) and refused(dk, dc, 8, 50, None, 4, good)
        assert refused(dk, dc, 8, 50, dx, 4, None)
        assert call(rfx, fn, dk, dc, 8, 50, dx, 4, good, None) == E_ARG
        for bad in (dict(min_error_cov=0), dict(min_repeat_fold=0.5), dict(max_k=0), dict(max_cov=-1)):
            assert refused(dk, dc, 8, 50, dx, 4, rfx.ksort_params(k, **bad)), bad
        for dtype, nbytes in ((np.int64, 8), (np.int32, 4)):
            counts = [5] * 50
            counts[37] = -1
            _, dneg = on_device(counter_words(kmers, k), counts, dtype)
            assert refused(dk, dneg, nbytes, 50, dx, 4, good), dtype
            assert b"negative count" in rfx.L.rfx_last_error(rfx.ctx)


def test_every_capacity_one_short(rfx):
    """capacities as rfx_dev_ksort_binarize's with n + n_extra for n_rows: one short gives RFX_E_CAP with n and need_words set and every
    output tensor as it was; the exact needs succeed; run_counts needs no extension words"""
    rng = np.random.default_rng(5)
    k = 41
    kmers = kmers_of(rng, k, 120)
    counts = [COUNTS[i % len(COUNTS)] for i in range(120)]
    dk, dc = on_device(counter_words(kmers, k), counts, np.int64)
    dx, _ = on_device(counter_words(kmers[:9], k))
    cp = rfx.ksort_params(k)
    for fn, words in ((rfx.L.rfx_dev_ksort_from_counts, True), (rfx.L.rfx_dev_ksort_run_counts, False)):
        big = poisoned(2 * 129, 2 * 129)
        co = big._c()
        assert call(rfx, fn, dk, dc, 8, 120, dx, 9, cp, co) == OK
        need_n, need_w = int(co.n), int(co.need_words)
        assert 0 < need_n <= 2 * 129 and need_w == (need_n if words else 0)
        assert call(rfx, fn, dk, dc, 8, 120, dx, 9, cp, poisoned(need_n, need_w)._c()) == OK
        for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
            if cap_w < 0:
                continue
            d = poisoned(cap_n, cap_w)
            co = d._c()
            co.n = co.need_words = -77
            assert call(rfx, fn, dk, dc, 8, 120, dx, 9, cp, co) == E_CAP
            assert (int(co.n), int(co.need_words)) == (need_n, need_w) and untouched(d)


def test_the_entry_points_hold_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is 0xA5 before the library uses it, so a producer that relied on zeroed
    memory for padding bits or unused key words fails the whole-word comparisons above.  A child process: the mask is read once"""
    import subprocess
    import sys
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
