"""The packed seams of the k-mer reduction (rfx_dev_reduce_union_packed, rfx_dev_reduce_run_packed) and of the hand-over to the
dynamic-k passes (rfx_dev_dyn_from_kmers); DESIGN.md section 32.  The expected set is always what the existing entry points give
through text: rfx_dev_reduce_union / rfx_dev_reduce_run on rfx_dev_ksort_to_text of the same two sets, and rfx_dev_dyn_binarize form
0 on the rows rfx_dev_ksort_to_text writes.  Sets are compared array by array, whole words."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_dynamic_packed import poisoned, untouched, OK, E_ARG, E_CAP
from tests.test_gpu_ksort import upload
from tests.test_gpu_ksort_counts import same_set, NUC

pytestmark = pytest.mark.gpu

PAIRS = ((23, 31), (31, 33), (31, 41), (62, 65), (93, 124))
PS = (1, 3, 8)
# what a set's int32 fields can hold and the text does something to: the clamp at +-30000 on both sides, nine and ten digits
WILD = (0, 1, -1, 98, 29999, 30000, 30001, -29999, -30000, -30001, 999_999_999, -999_999_999, 1_000_000_000, -1_000_000_000,
        1_234_567_891, 2**31 - 1, -2**31)


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


def rnd(rng, m):
    return "".join(NUC[b] for b in rng.integers(0, 4, m))


def count_rows(rng, k, length=330):
    """the `KMER,count` rows of a planted genome: one sequence at count 12, a copy with a substitution every 45 bases at count 3 (forks
    in both folds, error-corrected or not by their fold), and a few k-mers at count 1 (negative markers)"""
    g = rnd(rng, length)
    v = "".join(NUC[(NUC.index(c) + 1) % 4] if i % 45 == 22 else c for i, c in enumerate(g))
    rows = {}
    for seq, cnt in ((g, 12), (v, 3)):
        for i in range(len(seq) - k + 1):
            rows.setdefault(seq[i:i + k], cnt)
    for _ in range(20):
        rows.setdefault(rnd(rng, k), 1)
    return [f"{s},{c}\n" for s, c in sorted(rows.items())]


def sorted_set(rfx, seed, k, max_k):
    """Count_<k>_sorted of the planted genome of `seed`, as a packed set of full k-mers"""
    rows = count_rows(np.random.default_rng(seed), k)
    return rfx.ksort_run(*upload(rows), rfx.ksort_params(k, max_k=max_k))


def text_of(rfx, pk, k):
    d_text, ln, d_off, rows = rfx.ksort_to_text_dev(pk, k)
    return d_text[:ln], d_off[:rows + 1]


def crafted(rfx, rng, lengths, fields=None):
    """a packed set of full k-mers of the given key lengths (random bases); fields: what marker, left and right cycle through, written
    into the set's tensors as they are -- a set can hold what the host form would clamp"""
    import torch
    from reflexiv_amd.api import DynRecords
    n = len(lengths)
    r = DynRecords.from_text([rnd(rng, m) for m in lengths], [""] * n, [1] * n, [int(rng.integers(-40, 40)) for _ in range(n)],
                             [int(rng.integers(-40, 40)) for _ in range(n)])
    pk = rfx.dyn_pack(r)
    if fields and n:
        for j, t in enumerate((pk.marker, pk.left, pk.right)):
            t[:n] = torch.tensor([fields[(i + 5 * j) % len(fields)] for i in range(n)], dtype=torch.int32, device=t.device)
        torch.cuda.synchronize()
    return pk


# ---- 1. the union and the driver on the sorter's own output ---------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"k{p[0]}_{p[1]}")
def test_union_and_run_on_the_sorters_output_equal_the_text_path(rfx, pair):
    """both inputs are rfx_dev_ksort_run of a few hundred planted rows (forks, negative markers); P = 1, 3, 8; then the final set of
    the pair (k0, k1), which holds records of k0 AND k1 bases, as the short input of the pair (k1, k2): the k0 records must vanish"""
    k1, k2 = pair
    k0 = k1 - 4
    s0, s1, s2 = (sorted_set(rfx, 100 * k1 + k2, k, k2) for k in (k0, k1, k2))
    assert min(s0.n, s1.n, s2.n) > 200
    assert int((s1.left[:s1.n] < 0).sum()) + int((s1.right[:s1.n] < 0).sum()) > 0
    rp = rfx.reduce_params(k1, k2)
    t1, t2 = text_of(rfx, s1, k1), text_of(rfx, s2, k2)
    got = rfx.reduce_union_packed(s1, s2, rp)
    same_set(got, rfx.reduce_union(*t1, *t2, rp), (pair, "union"))
    assert got.n == s1.n + s2.n
    for P in PS:
        same_set(rfx.reduce_run_packed(s1, s2, P, rp), rfx.reduce_run(*t1, *t2, P, rp), (pair, P, "run"))
    # the chain: the pair before this one, then its final set as this pair's short input
    rp0 = rfx.reduce_params(k0, k1, max_k=k2)
    f01 = rfx.reduce_run_packed(s0, s1, 3, rp0)
    same_set(f01, rfx.reduce_run(*text_of(rfx, s0, k0), *t1, 3, rp0), (pair, "pair before"))
    assert set(f01.key_len[:f01.n].cpu().tolist()) <= {k0, k1}
    tf = text_of(rfx, f01, k1)
    got = rfx.reduce_union_packed(f01, s2, rp)
    same_set(got, rfx.reduce_union(*tf, *t2, rp), (pair, "union, chained"))
    assert set(got.key_len[:got.n].cpu().tolist()) == {k1, k2} and got.n <= f01.n + s2.n
    for P in (1, 8):
        same_set(rfx.reduce_run_packed(f01, s2, P, rp), rfx.reduce_run(*tf, *t2, P, rp), (pair, P, "run, chained"))


# ---- 2. sizes around the block, either side empty, fields beyond what the text keeps ---------------------------------------------------
@pytest.mark.parametrize("ns, nl", [(0, 0), (0, 257), (256, 0), (1, 1), (255, 257), (256, 256), (257, 255)])
def test_union_on_crafted_sets(rfx, ns, nl):
    """ns short and nl long records of the pair's lengths mixed with records of a third and a fourth length (dropped), markers and
    left / right cycling through +-30000, +-30001, nine and ten digits and the ends of int32"""
    for k1, k2 in ((31, 33), (62, 65), (93, 124)):
        rng = np.random.default_rng(1000 * ns + nl + k1)
        mix = lambda n, own, other: [own if i % 3 != 1 else (other, own - 1, own - 2)[(i // 3) % 3] for i in range(n)]
        s = crafted(rfx, rng, mix(ns, k1, k2), WILD)
        lg = crafted(rfx, rng, mix(nl, k2, k1), WILD)
        rp = rfx.reduce_params(k1, k2)
        got = rfx.reduce_union_packed(s, lg, rp)
        want = rfx.reduce_union(*text_of(rfx, s, k1), *text_of(rfx, lg, k2), rp)
        same_set(got, want, (ns, nl, k1, k2))
        assert got.n == sum(x == k1 for x in mix(ns, k1, k2)) + sum(x == k2 for x in mix(nl, k2, k1))
        if got.n:
            assert int(got.left[:got.n].max()) <= 30000 and int(got.right[:got.n].min()) >= -30000


def test_run_with_either_side_empty(rfx):
    k1, k2 = 31, 41
    s1, s2 = sorted_set(rfx, 9, k1, k2), sorted_set(rfx, 9, k2, k2)
    empty = crafted(rfx, np.random.default_rng(0), [])
    rp = rfx.reduce_params(k1, k2)
    for a, b in ((empty, s2), (s1, empty), (empty, empty)):
        for P in (1, 8):
            same_set(rfx.reduce_run_packed(a, b, P, rp), rfx.reduce_run(*text_of(rfx, a, k1), *text_of(rfx, b, k2), P, rp), (a.n, b.n, P))


# ---- 3. full k-mers -> the sub-k-mer records of the dynamic-k passes -------------------------------------------------------------------
def form0_of(rfx, sets, lens):
    """the text path: the rows of every (set, length) in order, concatenated, through rfx_dev_dyn_binarize form 0"""
    import torch
    texts, offs, base = [], [torch.zeros(1, dtype=torch.int64, device="cuda")], 0
    for pk, k in zip(sets, lens):
        t, o = text_of(rfx, pk, k)
        texts.append(t)
        offs.append(o[1:] + base)
        base += int(t.numel())
    d_text = torch.cat(texts) if base else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_off = torch.cat(offs)
    torch.cuda.synchronize()
    return rfx.dyn_binarize_dev(d_text, d_off, 0)


def test_dyn_from_kmers_one_set(rfx):
    """one set of two lengths, chosen in either order and one alone; the sorter's output and a crafted set whose left / right lie at
    +-30000 and beyond"""
    k1, k2 = 31, 41
    f = rfx.reduce_run_packed(sorted_set(rfx, 4, k1, k2), sorted_set(rfx, 4, k2, k2), 3, rfx.reduce_params(k1, k2))
    rng = np.random.default_rng(12)
    wild = crafted(rfx, rng, [(33, 65, 8, 124, 34)[i % 5] for i in range(600)], WILD)
    for pk, a, b in ((f, k1, k2), (wild, 33, 124), (wild, 8, 65)):
        for lens in ((a,), (a, b), (b, a), (b, b)):
            got = rfx.dyn_from_kmers([pk] * len(lens), lens)
            same_set(got, form0_of(rfx, [pk] * len(lens), lens), (a, b, lens))
            assert got.n > 0 and set(got.marker[:got.n].cpu().tolist()) == {1}
    got = rfx.dyn_from_kmers([wild], [33])
    assert int(got.left[:got.n].max()) == 30000 and int(got.left[:got.n].min()) == -30000
    assert rfx.dyn_from_kmers([wild], [50]).n == 0 and rfx.dyn_from_kmers([], []).n == 0


def test_dyn_from_kmers_three_sets(rfx):
    """the chain's hand-over: the k0 records of pair (k0, k1), then the k1 and the k2 records of pair (k1, k2) -- the list (23, 31, 41)"""
    k0, k1, k2 = 23, 31, 41
    s0, s1, s2 = (sorted_set(rfx, 21, k, k2) for k in (k0, k1, k2))
    f01 = rfx.reduce_run_packed(s0, s1, 8, rfx.reduce_params(k0, k1, max_k=k2))
    f12 = rfx.reduce_run_packed(f01, s2, 8, rfx.reduce_params(k1, k2))
    sets, lens = [f01, f12, f12], [k0, k1, k2]
    got = rfx.dyn_from_kmers(sets, lens)
    same_set(got, form0_of(rfx, sets, lens), "three sets")
    assert set(got.key_len[:got.n].cpu().tolist()) == {k0 - 1, k1 - 1, k2 - 1}
    # an empty set in the middle, and the block edge: 255, 0, 257 records
    rng = np.random.default_rng(2)
    sets = [crafted(rfx, rng, [62] * 255, WILD), crafted(rfx, rng, []), crafted(rfx, rng, [95] * 257, WILD)]
    same_set(rfx.dyn_from_kmers(sets, [62, 65, 95]), form0_of(rfx, sets, [62, 65, 95]), "255 + 0 + 257")


# ---- 4. contracts ------------------------------------------------------------------------------------------------------------------------
def test_capacities_and_refused_arguments(rfx):
    k1, k2 = 31, 41
    s1, s2 = sorted_set(rfx, 33, k1, k2), sorted_set(rfx, 33, k2, k2)
    c1, c2 = s1._c(), s2._c()
    rp = rfx.reduce_params(k1, k2)
    L, ctx = rfx.L, rfx.ctx
    arr = (type(c1) * 2)(s1._c(), s2._c())
    lens = (C.c_int * 2)(k1, k2)
    ops = {"union": lambda co: L.rfx_dev_reduce_union_packed(ctx, C.byref(c1), C.byref(c2), C.byref(rp), C.byref(co)),
           "run": lambda co: L.rfx_dev_reduce_run_packed(ctx, C.byref(c1), C.byref(c2), 3, C.byref(rp), C.byref(co)),
           "from_kmers": lambda co: L.rfx_dev_dyn_from_kmers(ctx, C.addressof(arr), C.addressof(lens), 2, C.byref(co))}
    for name, call in ops.items():
        big = poisoned(s1.n + s2.n, s1.n + s2.n)
        co = big._c()
        assert call(co) == OK, name
        need_n, need_w = int(co.n), int(co.need_words)
        assert need_n > 0 and need_w == (need_n if name == "from_kmers" else 0), name
        assert call(poisoned(need_n, need_w)._c()) == OK, name
        for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
            if cap_w < 0:
                continue
            d = poisoned(cap_n, cap_w)
            co = d._c()
            co.n = co.need_words = -77
            assert call(co) == E_CAP, (name, cap_n, cap_w)
            assert (int(co.n), int(co.need_words)) == (need_n, need_w) and untouched(d), name
    d = poisoned(s1.n + s2.n, s1.n + s2.n)
    co = d._c()
    bad_pair = rfx.reduce_params(41, 31)
    no_key = s1._c()
    no_key.key = None
    assert L.rfx_dev_reduce_union_packed(ctx, C.byref(c1), C.byref(c2), C.byref(bad_pair), C.byref(co)) == E_ARG
    assert L.rfx_dev_reduce_union_packed(ctx, None, C.byref(c2), C.byref(rp), C.byref(co)) == E_ARG
    assert L.rfx_dev_reduce_union_packed(ctx, C.byref(c1), C.byref(no_key), C.byref(rp), C.byref(co)) == E_ARG
    assert L.rfx_dev_reduce_union_packed(ctx, C.byref(c1), C.byref(c2), None, C.byref(co)) == E_ARG
    assert L.rfx_dev_reduce_union_packed(ctx, C.byref(c1), C.byref(c2), C.byref(rp), None) == E_ARG
    for P in (0, 64, -1):
        assert L.rfx_dev_reduce_run_packed(ctx, C.byref(c1), C.byref(c2), P, C.byref(rp), C.byref(co)) == E_ARG
    assert L.rfx_dev_reduce_run_packed(ctx, C.byref(c1), None, 3, C.byref(rp), C.byref(co)) == E_ARG
    assert L.rfx_dev_dyn_from_kmers(ctx, None, C.addressof(lens), 2, C.byref(co)) == E_ARG
    assert L.rfx_dev_dyn_from_kmers(ctx, C.addressof(arr), None, 2, C.byref(co)) == E_ARG
    assert L.rfx_dev_dyn_from_kmers(ctx, C.addressof(arr), C.addressof(lens), -1, C.byref(co)) == E_ARG
    assert L.rfx_dev_dyn_from_kmers(ctx, C.addressof(arr), C.addressof(lens), 65, C.byref(co)) == E_ARG
    assert L.rfx_dev_dyn_from_kmers(ctx, C.addressof(arr), C.addressof(lens), 2, None) == E_ARG
    for bad in (0, 125, -3):
        bl = (C.c_int * 2)(k1, bad)
        assert L.rfx_dev_dyn_from_kmers(ctx, C.addressof(arr), C.addressof(bl), 2, C.byref(co)) == E_ARG
    assert untouched(d)


def test_the_seams_hold_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is 0xA5 before the library uses it -- the new code writes the padding
    bits and the unused key words itself.  A child process: the mask is read once per process"""
    import os
    import subprocess
    import sys
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
