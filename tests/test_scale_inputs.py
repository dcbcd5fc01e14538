"""The inputs and the numpy checkers of tests/test_gpu_dynamic_scale.py, on the CPU: its vectorised statements of the model (sort
order, partition starts, the raw-word packer, the pending-row trace) against the model itself on small sets, and every generator
against the conditions its test relies on, at the seed and size the GPU test uses.  Needs no GPU."""
import numpy as np

from tests import pymodel as M
from tests import reduce_model as R
from tests import test_gpu_dynamic_scale as S
from tests.test_gpu_dynamic_packed import np_packed, records_of, KEY_LENGTHS, EXT_LENGTHS
from tests.test_gpu_reduce import crafted_rows
from tests.test_oracle_dynamic import model_rows


def mixed_records(rng, n):
    """records_of's keys of 1..124 bases, every fourth key a prefix of the one before and every fifth a copy; one key is G A^30 G:
    its first block is the smallest long, ahead of a one-block key G A^30 ... of more bases"""
    r = records_of(rng, n)
    recs = S.tuples_of(r, "dyn")
    for i in range(1, n):
        if i % 4 == 0:
            recs[i] = (recs[i - 1][0][:1 + int(rng.integers(0, len(recs[i - 1][0])))],) + recs[i][1:]
        elif i % 5 == 0:
            recs[i] = (recs[i - 1][0],) + recs[i][1:]
    recs[7] = ("G" + "A" * 30 + "G",) + recs[7][1:]
    recs[8] = ("G" + "A" * 30,) + recs[8][1:]
    recs[9] = ("G" + "A" * 29,) + recs[9][1:]
    return recs


def test_the_numpy_sort_order_and_partition_starts_are_the_models():
    recs = mixed_records(np.random.default_rng(1), 5000)
    r = S.host_dyn(recs)
    want = M.dyn_sort(recs)
    got = S.take(r, S.sort_order(r))
    assert got.rows() == model_rows(want)
    assert S.tuples_of(got, "dyn") == want
    for P in (1, 2, 7, 63):
        assert S.partition_starts_np(got, P) == M.dyn_partition_starts(want, P), P
    # a set of few keys: the cut moves far forward and partitions come out empty
    few = [(("ACGT" * 31)[:1 + i % 3], 1, "A", i, i) for i in range(100)]
    fr = S.host_dyn(few)
    fs = S.take(fr, S.sort_order(fr))
    assert S.tuples_of(fs, "dyn") == M.dyn_sort(few)
    assert S.partition_starts_np(fs, 7) == M.dyn_partition_starts(M.dyn_sort(few), 7)


def test_the_vectorised_packer_is_np_packed():
    from reflexiv_amd.api import DynRecords
    for r in (records_of(np.random.default_rng(2), 700), S.pack_records(20_007), DynRecords.from_rows([]),
              S.take(S.sort_records(30_000, True), np.arange(3000))):
        r = S.take(r, np.arange(min(r.n, 1500))) if r.n else r
        for name, a, b in zip(("key", "key_len", "ext", "ext_off", "ext_len"), S.np_packed_fast(r), np_packed(r)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, r.n)
    # take and concat keep the records
    r = records_of(np.random.default_rng(3), 300)
    sel = np.random.default_rng(3).permutation(300)
    rows = r.rows()
    assert S.take(r, sel).rows() == [rows[i] for i in sel]
    assert S.concat(S.take(r, np.arange(100)), S.take(r, np.arange(100, 300))).rows() == rows


def test_the_pack_records_hold_every_class():
    for n in (4096, 270_000):
        r = S.pack_records(n)
        pairs = np.unique(np.stack([np.diff(r.key_off), np.diff(r.ext_off)]), axis=1, return_counts=True)
        assert {(int(a), int(b)) for a, b in pairs[0].T} == {(a, b) for a in KEY_LENGTHS for b in EXT_LENGTHS}
        assert r.n == n and set(np.unique(r.key)) == {0, 1, 2, 3} == set(np.unique(r.ext)) and set(np.unique(r.marker)) == {1, 2}
    big = np.diff(S.pack_records(270_000).ext_off) == 1000
    assert big.sum() == 270_000 // 9 // 50 == 600


def test_the_pending_trace_is_the_models_loop():
    """on 3,000 rows of the crafted input: the rows the trace says the loop writes are the rows reduce_model.adjust writes, for
    every prefix length that ends a different way (so a miscounted state shows at the flush), in both directions"""
    rs, rl = crafted_rows(np.random.default_rng(9), *S.REDUCE_K, groups=900)
    st, _ = R.run_stages(rs, rl, *S.REDUCE_K, 1)
    for right, name in ((False, "left_sort"), (True, "right_sort")):
        recs = st[name][:3000]
        assert len(recs) == 3000
        ahead, written = S.pending_trace(recs, right, S.REDUCE_K[0])
        assert written == len(R.adjust(recs, right, S.REDUCE_K[0])) and set(ahead) == {0, 1, 2}
        for n in list(range(0, 40)) + list(range(2960, 3000)):
            a, w = S.pending_trace(recs[:n], right, S.REDUCE_K[0])
            assert a == ahead[:n] and w == len(R.adjust(recs[:n], right, S.REDUCE_K[0])), (right, n)


def test_the_reduce_input_holds_every_pending_count_at_the_block_starts():
    run = S.reduce_model_run()
    for right, name in ((False, "left_sort"), (True, "right_sort")):
        recs = run["st"][name]
        assert len(recs) >= S.REDUCE_MIN_ROWS, (name, len(recs))
        ahead, written = S.pending_trace(recs, right, S.REDUCE_K[0])
        counts, changes, starts = S.state_variety(ahead)
        print(name, len(recs), "pending 0/1/2 at the block starts:", counts, "changes:", changes, "of", starts)
        assert min(counts) >= 2 and 5 * changes >= starts and S.variety_holds(ahead), (name, counts, changes, starts)
        assert starts == len(range(65_536, len(recs), 256)) >= 258
    assert [S.reduce_starts(n) for n in (65_536, 65_537, 131_073)] == [[0, 65_536], [0, 65_536, 65_537], [0, 65_536, 65_537, 100_000, 131_072, 131_073]]


def test_the_sort_inputs_have_the_stated_buckets_duplicates_and_block_counts():
    for n, skewed in S.SORT_CASES:
        r = S.sort_records(n, skewed)
        assert r.n == n
        ln = np.diff(r.key_off)
        assert ln.min() == 1 and ln.max() == 124 and set(np.unique((ln + 30) // 31)) == {1, 2, 3, 4}
        top = S.top16_histogram_max(r)
        assert (top > S.SORT_TILE) if skewed else (top < S.SORT_TILE), (n, skewed, top)
        # the 2,000 duplicated keys: 3 to 6 records each, their extensions of different lengths
        cols, nb = S.block_columns(r)
        long_keys = np.flatnonzero(ln >= 16)
        k = np.stack(cols + [nb])[:, long_keys]
        _, inv, cnt = np.unique(k, axis=1, return_inverse=True, return_counts=True)
        assert (cnt > 1).sum() == S.SORT_DUP_KEYS and set(cnt[cnt > 1]) == {3, 4, 5, 6}
        el = np.diff(r.ext_off)[long_keys]
        inv = np.asarray(inv).reshape(-1)
        assert len(np.unique(inv.astype(np.int64) * 8 + el)) == len(inv)
        if skewed:
            first8 = r.key[np.add.outer(r.key_off[:-1][ln >= 9], np.arange(8))]
            assert (first8 == S.SORT_SKEW_PREFIX).all(axis=1).sum() >= S.SORT_SKEW_KEYS
    assert S.SORT_CASES[0][0] == 192 * S.SORT_TILE and S.SORT_CASES[1][0] > 192 * S.SORT_TILE


def test_the_pass_and_ksort_inputs_have_the_stated_sizes():
    recs = S.pass_records()
    assert 65_000 < len(recs) < 75_000 and {len(r[0]) for r in recs} == set(M.DYN_WIDE_LENGTHS) and {r[1] for r in recs} == {1, 2}
    for k in (31, 95):
        rows = S.ksort_rows(k)
        assert 68_000 < len(rows) < 72_000 and all(len(row.split(",")[0]) == k for row in rows[:50])


def test_the_fork_filter_input_has_every_run_kind_and_runs_across_the_edges():
    for reflected in (False, True):
        recs, runs = S.fork_records(reflected)
        assert len(recs) == S.FORK_N and {r[1] for r in recs} == {2 if reflected else 1} and {len(r[0]) for r in recs} == {30}
        r = S.host_dyn(recs)
        assert np.array_equal(S.sort_order(r), np.arange(r.n))
        assert len(runs) >= S.FORK_RUNS and {ln for _, ln, _ in runs} == set(range(2, 41))
        kinds = {}
        for first, ln, kind in runs:
            kinds[kind] = kinds.get(kind, 0) + 1
            assert len({rec[0] for rec in recs[first:first + ln]}) == 1 and recs[first - 1][0] != recs[first][0]
            assert first + ln == S.FORK_N or recs[first + ln][0] != recs[first][0]
        assert set(kinds) == set(S.FORK_KINDS) and min(kinds.values()) >= 700
        for edge in S.FORK_EDGES:
            assert any(first + 2 <= edge <= first + ln - 2 for first, ln, _ in runs), edge
        # each kind as the 600-row test states it
        for first, ln, kind in runs[:400]:
            ext = [len(rec[2]) for rec in recs[first:first + ln]]
            if kind in ("ones", "ties"):
                assert max(ext) == 1
            elif kind == "ones then longs":
                assert ext[0] == 1 and ext[-1] > 1 and sorted(x > 1 for x in ext) == [x > 1 for x in ext]
            else:
                assert ext[-1] > 1 and (ln < 3 or 1 in ext)


def test_the_kmer_set_input_has_the_stated_duplicates():
    v, longs = S.kmer_set_input()
    assert len(v) == S.KMER_SET_N and len(np.unique(v)) == S.KMER_SET_N - S.KMER_SET_DUPS and v.min() >= 0 and v.max() < 1 << 62
    assert len(longs) == S.KMER_SET_LONGS and all(len(r[0]) == 30 and len(r[2]) >= 2 for r in longs)
    assert S.KMER_SET_N > 192 * S.SORT_TILE
    want, distinct = S.kmer_set_records(v[:2000], longs)
    from tests import fixing_model as F
    from tests.test_gpu_fixing import value_of
    kmers = ["".join("ACGT"[(int(x) >> (60 - 2 * j)) & 3] for j in range(31)) for x in v[:2000]]
    assert [value_of(k) for k in kmers] == v[:2000].tolist()
    assert S.tuples_of(want, "dyn") == F.kmer_set(kmers, longs, "sorted") and distinct == len(set(kmers))
