"""Two-word k-mers (k = 33..63) through the element path that W = 3, 4 use: level 1 straight from the packed reads
(k_wn_hist<2> / k_wn_scatter<2>, 16 ring slots per bin), the record levels on KmerW<2>, and the W-word leaf at W = 2, which
claims a slot by a compare-and-swap on each of its two key words.  From reads this path runs under RFX_WIDE_RECORDS=0 (uniform lengths only: ragged reads
always take the super-k-mer records); rfx_dev_count_wide_elems, rfx_count_filter_w and rfx_dev_bucket_wide_by_owner always
use it.  Everything against the oracle's k > 31 counter; bit-exact (integer work)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_dist_gloo import mulhi_owner, wide_hash
from tests.test_gpu_count_w34 import COMP, reads_of, rfx, t_and_a_run_reads, torch_mod  # noqa: F401  (rfx, torch_mod: fixtures)
from tests.test_gpu_ragged_w import upload

pytestmark = pytest.mark.gpu

BIG = 10_000_000
EDGE_KS = (33, 34, 47, 62, 63)          # last word of 1, 2, 15, 30, 31 bases; k = 33: the 2 * (res - 1) shifts are zero


@pytest.fixture(scope="module")
def genome():
    return "".join(np.random.default_rng(2024).choice(list("ACGT"), size=2000))


def uniform_reads(genome, L, n_reads, seed, err=0.0):
    """n_reads reads of L bases cut from the genome, either strand, with substitutions at rate err"""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n_reads):
        p = int(rng.integers(0, len(genome) - L + 1))
        s = list(genome[p:p + L])
        for j in np.nonzero(rng.random(L) < err)[0]:
            s[j] = "ACGT"[("ACGT".index(s[j]) + int(rng.integers(1, 4))) % 4]
        reads.append("".join(s) if rng.random() < 0.5 else "".join(COMP[c] for c in reversed(s)))
    return reads_of(reads)


def count_uniform(rfx, torch, bases, off, k, min_cov=1, max_cov=BIG):
    """rfx_dev_count_reads_w on reads of one length -> (m, n_distinct, instances, keys[m, 2], counts[m])"""
    dw, _, n, wpr, L = upload(rfx, torch, bases, off)
    cap = max(1, rfx.kmers_per_read_w(L, k) * n)
    dk = torch.empty(2 * cap, dtype=torch.int64, device="cuda")
    dc = torch.empty(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m, nd, inst = rfx.count_reads_w_dev(dw.data_ptr(), n, wpr, L, k, dk.data_ptr(), dc.data_ptr(), cap, min_cov, max_cov)
    return m, nd, inst, dk[:2 * m].cpu().numpy().view(np.uint64).reshape(m, 2), dc[:m].cpu().numpy()


def check_uniform(rfx, torch, bases, off, k, min_covs=(1, 2), km=None):
    km = O.extract_canon_w(bases, off, k) if km is None else km
    for min_cov in min_covs:
        m, nd, inst, keys, counts = count_uniform(rfx, torch, bases, off, k, min_cov)
        wk, wc, wd = O.count_filter_w(km, k, min_cov)
        assert (inst, nd, m) == (len(km), wd, len(wk)), (k, min_cov)
        assert np.array_equal(keys, wk) and np.array_equal(counts, wc), (k, min_cov)
    return km


def count_elems(rfx, torch, km, k, min_cov=1, max_cov=BIG):
    """rfx_dev_count_wide_elems on AoS two-word elements -> (m, n_distinct, keys[m, 2], counts[m])"""
    n = len(km)
    de = torch.from_numpy(np.ascontiguousarray(km, np.uint64).view(np.int64).reshape(-1).copy() if n else np.zeros(2, np.int64)).cuda()
    dk = torch.empty(2 * max(1, n), dtype=torch.int64, device="cuda")
    dc = torch.empty(max(1, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m, nd = rfx.count_wide_elems_dev(de.data_ptr(), n, k, dk.data_ptr(), dc.data_ptr(), max(1, n), min_cov, max_cov)
    return m, nd, dk[:2 * m].cpu().numpy().view(np.uint64).reshape(m, 2), dc[:m].cpu().numpy()


def check_elems(rfx, torch, km, k, min_cov, max_cov=BIG):
    m, nd, keys, counts = count_elems(rfx, torch, km, k, min_cov, max_cov)
    wk, wc, wd = O.count_filter_w(km, k, min_cov, max_cov)
    assert (nd, m) == (wd, len(wk)), (k, min_cov, max_cov)
    assert np.array_equal(keys, wk) and np.array_equal(counts, wc), (k, min_cov, max_cov)


def distinct_kmers(k, n, seed):
    """n distinct canonical two-word k-mers from the oracle (so no word is all ones), in random order"""
    rng = np.random.default_rng(seed)
    bases, off = reads_of(["".join(rng.choice(list("ACGT"), size=2 * n + k))])
    km = np.unique(O.extract_canon_w(bases, off, k), axis=0)
    assert len(km) >= n and not (km == np.uint64(0xFFFFFFFFFFFFFFFF)).any()
    return km[rng.permutation(len(km))[:n]]


@pytest.mark.parametrize("k", EDGE_KS)
@pytest.mark.parametrize("extra", [0, 1, 15, 16, 17])
def test_level1_at_the_segment_edges(rfx, torch_mod, genome, k, extra, monkeypatch):
    """a thread of level 1 owns 16 windows: reads of k + extra bases have 1, 2, 16, 17 and 18 windows, so the last segment
    is full, holds one window, or two"""
    monkeypatch.setenv("RFX_WIDE_RECORDS", "0")
    bases, off = uniform_reads(genome, k + extra, 300, 100 * k + extra)
    assert rfx.kmers_per_read_w(k + extra, k) == extra + 1
    km = check_uniform(rfx, torch_mod, bases, off, k)
    assert len(km) == 300 * (extra + 1) and len(np.unique(km, axis=0)) < len(km)        # repeats occur


@pytest.mark.parametrize("k", [33, 63])
@pytest.mark.parametrize("owners", [1, 3, 64])
def test_owner_buckets_at_the_segment_edges(rfx, torch_mod, genome, k, owners):
    """every element lies in the bucket of mulhi(wide_hash(word0, word1), owners), and the buckets hold the oracle's k-mers"""
    torch = torch_mod
    L = k + 17
    bases, off = uniform_reads(genome, L, 300, 7 * k + owners)
    dw, _, n, wpr, _ = upload(rfx, torch, bases, off)
    km = O.extract_canon_w(bases, off, k)
    N = len(km)
    out = torch.empty(2 * N, dtype=torch.int64, device="cuda")
    doff = torch.empty(owners + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h = rfx.bucket_wide_by_owner_dev(dw.data_ptr(), n, wpr, L, k, owners, out.data_ptr(), N, doff.data_ptr())
    assert h[0] == 0 and h[-1] == N and np.all(np.diff(h) >= 0) and np.array_equal(h, doff.cpu().numpy())
    got = out.cpu().numpy().view(np.uint64).reshape(N, 2)
    assert np.array_equal(mulhi_owner(wide_hash(got[:, 0], got[:, 1]), owners), np.repeat(np.arange(owners), np.diff(h)))
    assert np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], km[np.lexsort((km[:, 1], km[:, 0]))])


@pytest.mark.parametrize("k", [33, 63])
def test_leaf_table_one_leaf(rfx, torch_mod, k):
    """3,000 distinct keys, each twice: one leaf, whose 4096-slot table takes them without an overflow (a probe sequence
    of LPROBE = 48 slots at a load of 0.73 fails with probability 0.73^48 < 1e-6 per key)"""
    km = distinct_kmers(k, 3000, k)
    km = np.concatenate([km, km[::-1]])
    for min_cov in (1, 2, 3):
        check_elems(rfx, torch_mod, km, k, min_cov)
    t = rfx.count_timing()
    assert t["stat_leaves"][1] == 1 and t["stat_passes"][1] == 1 and t["stat_overflows"][1] == 0, t


@pytest.mark.parametrize("k", [33, 63])
def test_leaf_table_overflows_and_splits(rfx, torch_mod, k):
    """6,000 distinct keys in one leaf: more than the table's 4096 slots, so the pass is abandoned and the leaf splits"""
    km = distinct_kmers(k, 6000, k + 1)
    check_elems(rfx, torch_mod, km, k, 1)
    t = rfx.count_timing()
    assert t["stat_leaves"][1] == 1 and t["stat_overflows"][1] > 0 and t["stat_passes"][1] > 2, t
    check_elems(rfx, torch_mod, km, k, 2)            # nothing survives


@pytest.mark.parametrize("k", [33, 63])
def test_leaf_table_one_heavy_key(rfx, torch_mod, k):
    """one key 200,000 times among 1,000 singletons: every count add lands with a whole workgroup claiming one slot"""
    km = distinct_kmers(k, 1001, k + 2)
    km = np.concatenate([np.repeat(km[:1], 200_000, axis=0), km[1:]])
    km = km[np.random.default_rng(k).permutation(len(km))]
    check_elems(rfx, torch_mod, km, k, 1)
    check_elems(rfx, torch_mod, km, k, 2)
    check_elems(rfx, torch_mod, km, k, 1, max_cov=199_999)


@pytest.mark.parametrize("k", [33, 63])
def test_leaf_table_one_element_and_none(rfx, torch_mod, k):
    km = distinct_kmers(k, 1, k + 3)
    check_elems(rfx, torch_mod, km, k, 1)
    check_elems(rfx, torch_mod, km, k, 2)
    assert count_elems(rfx, torch_mod, km[:0], k)[:2] == (0, 0)


@functools.lru_cache(maxsize=None)
def forced_plan_reads():
    """the read-set size of test_leaf_tables_under_forced_plans: 8000 reads (of 150 bases) from 40,000"""
    genome = "".join(np.random.default_rng(55).choice(list("ACGT"), size=40_000))
    return uniform_reads(genome, 150, 8000, 56, err=0.02)


@functools.lru_cache(maxsize=None)
def forced_plan_kmers(k):
    return O.extract_canon_w(*forced_plan_reads(), k)


@pytest.mark.parametrize("k", [47, 63])
@pytest.mark.parametrize("env", [{"RFX_LEVEL_BITS": "4,3,3"},
                                 {"RFX_LEAF_TARGET": "200000", "RFX_WIDE_PRESPLIT": "64"},
                                 {"RFX_LEAF_TARGET": "200000", "RFX_WIDE_PRESPLIT": "100000000"}])
def test_leaf_tables_under_forced_plans_w2(rfx, torch_mod, env, k, monkeypatch):
    """test_leaf_tables_under_forced_plans (tests/test_gpu_count_w34.py) on two-word elements: a distinct-heavy set (2 %
    substitutions) under several levels, leaves far beyond one table started in parts, and the same leaves found too full
    one pass at a time"""
    monkeypatch.setenv("RFX_WIDE_RECORDS", "0")
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    bases, off = forced_plan_reads()
    check_uniform(rfx, torch_mod, bases, off, k, min_covs=(1,), km=forced_plan_kmers(k))
    t = rfx.count_timing()
    if "RFX_LEAF_TARGET" in env:
        assert t["stat_passes"][1] > t["stat_leaves"][1] and t["stat_overflows"][1] > 0, t
    else:
        assert t["stat_leaves"][1] == 1 << 10 and t["stat_passes"][1] >= t["stat_leaves"][1], t


@pytest.mark.parametrize("k", [33, 63])
def test_runs_of_t_and_a_through_the_element_path(rfx, torch_mod, k, monkeypatch):
    """the reads of test_all_ones_and_all_zeros_middle_words at one length: word 0 is all zeros (32 A's) in some keys and
    word 1 all T's (its largest value, never all ones) in others: no key word equals the table's EMPTY (all ones), which
    the leaf's word-by-word claim at W = 2 relies on, and keys that agree in one word share no slot"""
    monkeypatch.setenv("RFX_WIDE_RECORDS", "0")
    bases, off = t_and_a_run_reads(k, uniform_len=200)
    km = check_uniform(rfx, torch_mod, bases, off, k)
    assert (km[:, 0] == 0).any() and (km[:, 1] == np.uint64((1 << (2 * (k - 32))) - 1)).any()
    assert (km[:, 1] == 0).any() and not (km == np.uint64(0xFFFFFFFFFFFFFFFF)).any()
    # the same k-mers as device elements and as host arrays (rfx_count_filter_w: the count straight from AoS elements)
    check_elems(rfx, torch_mod, km, k, 1)
    keys, counts, nd = rfx.groupBy_count_filter_w(km, k, 1)
    wk, wc, wd = O.count_filter_w(km, k, 1)
    assert np.array_equal(np.asarray(keys).reshape(-1, 2), wk) and np.array_equal(np.asarray(counts), wc) and nd == wd
