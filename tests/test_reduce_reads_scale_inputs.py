"""The inputs and the numpy statements of tests/test_gpu_reduce_reads_scale.py, on the CPU: every numpy restatement against its string
model on a few thousand mixed records, every generator against the conditions its test relies on at the seed and size the GPU test
uses, and the driver's read set against every condition that decided its genome size.  Needs no GPU."""
import numpy as np
import pytest

from tests import ksort_model as K
from tests import reduce_model as R
from tests import reduce_reads_model as RR
from tests import test_gpu_dynamic_scale as S
from tests import test_gpu_reduce_reads_scale as T
from tests.test_gpu_ksort_counts import counter_words, MAX_COV

K1, K2 = S.REDUCE_K


def tiles(flags):
    """a flag per row -> the rows of each 4,096-row tile"""
    return [flags[i:i + T.TILE] for i in range(0, len(flags), T.TILE)]


def every_tile_has(flags):
    return all(t.any() for t in tiles(flags))


def no_period_of_a_tile(flags):
    """no two full tiles hold their flags at the same places"""
    full = [t.tobytes() for t in tiles(flags) if len(t) == T.TILE]
    return len(set(full)) == len(full)


# ---- the numpy statements against the string models ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 23, 31, 33, 41, 65, 95, 124])
def test_the_numpy_counter_words_are_counter_words(k):
    rng = np.random.default_rng(k)
    codes = rng.integers(0, 4, (500, k), dtype=np.uint8)
    kmers = T.kmer_strings(codes)
    assert [len(s) for s in kmers] == [k] * 500 and np.array_equal(T.kmer_codes(kmers, k), codes)
    plain = counter_words(kmers, k)
    assert np.array_equal(T.counter_words_np(codes, k), plain)
    junk = T.counter_words_np(codes, k, np.random.default_rng(1))
    m = k % 32
    low = np.uint64((1 << (2 * m)) - 1)
    assert np.array_equal(junk[:, :-1], plain[:, :-1]) and np.array_equal(junk[:, -1] & low, plain[:, -1])
    assert ((junk[:, -1] & ~low) != 0).sum() > 300 and RR.key_letters(plain[7], k) == kmers[7]


@pytest.mark.parametrize("k", [23, 31, 41, 65, 95])
def test_the_numpy_binarize_is_the_models(k):
    """3,000 solid and 500 extra rows; the counts of the GPU test and counts of ten digits and more, which read as 1,000,000,000"""
    rng = np.random.default_rng(k)
    codes = rng.integers(0, 4, (3500, k), dtype=np.uint8)
    counts = rng.choice(np.concatenate([T.KEPT_COUNTS, T.DROPPED_COUNTS, [0, 1_000_000_000, 2**31 - 1, 2**40]]), 3000).astype(np.int64)
    rows = T.count_rows(codes, counts)
    assert len(rows) == 3500 and rows[3000].endswith(",1\n")
    for max_cov in (MAX_COV, 2**31 - 1, 0):
        want = K.binarize(rows, K.default_params(k, max_cov=max_cov))
        got = T.binarize_np(codes, counts, k, max_cov)
        assert S.tuples_of(got, "kmer") == want and (max_cov == 0 or len(want) > 1000), (k, max_cov)


def mixed_sets(seed, n_short, n_long):
    rng = np.random.default_rng(seed)
    lens = [K1, K2, T.FOREIGN_LEN, K1 - 1, K2 + 1]
    return T.kmer_set_np(rng, rng.choice(lens, n_short)), T.kmer_set_np(rng, rng.choice(lens, n_long))


def test_the_numpy_union_is_the_models_on_the_two_texts():
    for seed, ns, nl in ((1, 3000, 4000), (2, 0, 500), (3, 500, 0)):
        short, long = mixed_sets(seed, ns, nl)
        ts, tl = S.tuples_of(short, "kmer"), S.tuples_of(long, "kmer")
        want = R.union(R.to_text(ts, K1).splitlines(), R.to_text(tl, K2).splitlines(), K1, K2)
        got = T.union_np(short, long, K1, K2)
        assert S.tuples_of(got, "kmer") == want and got.n == sum(len(r[0]) == K1 for r in ts) + sum(len(r[0]) == K2 for r in tl)
    short, _ = mixed_sets(1, 3000, 1)
    assert {-T.CLAMP, T.CLAMP} <= set(short.left.tolist()) and {-T.CLAMP, T.CLAMP} <= set(short.right.tolist())


def test_the_numpy_handover_is_both_models_and_the_pinned_form():
    short, _ = mixed_sets(4, 4000, 1)
    recs = S.tuples_of(short, "kmer")
    for k in (K1, K2, T.FOREIGN_LEN, 50):
        text = R.to_text(recs, k)
        want = R.handover(text)
        assert want == K.handover(text) == [(r[0][:-1], r[0][-1], 1, r[3], r[4]) for r in recs if len(r[0]) == k]
        assert S.tuples_of(T.handover_np(short, k), "kmer") == want and (len(want) > 500 or k == 50)


def test_with_foreign_keeps_the_order_of_the_own_records():
    own = T.kmer_set_np(np.random.default_rng(5), np.full(5000, K1))
    mixed = T.with_foreign(own, 5)
    ln = T.key_lengths(mixed)
    assert set(ln.tolist()) == {K1, T.FOREIGN_LEN} and int((ln == T.FOREIGN_LEN).sum()) == 5000 // (T.FOREIGN_ONE_IN - 1) + 8
    assert S.tuples_of(T.select_np(mixed, K1), "kmer") == S.tuples_of(own, "kmer")


# ---- a drop or a foreign record in every tile -----------------------------------------------------------------------------------------------
def test_the_counter_inputs_drop_a_row_in_every_tile_of_solid_rows():
    """an extra row's count is 1, so a tile of extra rows alone holds no drop: the seam at 4,000 leaves such tiles at 8,193 and at 270,000
    rows, which is why (12000, 290) is run too; behind a tile with a drop no rank is its row number any more"""
    for k in T.COUNT_KS + (T.COUNT_LARGE[2],):
        for n, n_extra in T.COUNT_CASES + (T.COUNT_LARGE[:2],):
            if (k == T.COUNT_LARGE[2]) != ((n, n_extra) == T.COUNT_LARGE[:2]):
                continue
            codes, counts = T.counts_input(n, n_extra, k)
            assert codes.shape == (n + n_extra, k) and len(counts) == n and counts.min() >= 1
            drop = counts > MAX_COV
            assert every_tile_has(drop) and no_period_of_a_tile(drop), (k, n, n_extra)
            assert set(counts[drop].tolist()) == set(T.DROPPED_COUNTS.tolist()) and set(counts[~drop].tolist()) == set(T.KEPT_COUNTS.tolist())
            assert len(set(T.kmer_strings(codes[:2000]))) == 2000
    assert [n + x for n, x in T.COUNT_CASES] == [4096, 4097, 8193, 12_290] and sum(T.COUNT_LARGE[:2]) == 270_000 > 64 * T.TILE
    assert T.COUNT_CASES[0][0] < T.TILE < 2 * T.TILE < T.COUNT_CASES[3][0] and T.COUNT_LARGE[0] > 63 * T.TILE
    assert 68_000 < len(S.ksort_rows(31)) < 72_000 and max(S.TK.COUNTS) <= MAX_COV


def test_the_packed_inputs_hold_a_foreign_record_in_every_tile():
    inp = T.packed_inputs()
    rs, rl = S.reduce_rows()
    for name, rows, own_len in (("short", rs, K1), ("long", rl, K2)):
        r = inp[name]
        ln = T.key_lengths(r)
        foreign = ln == T.FOREIGN_LEN
        assert set(ln.tolist()) == {own_len, T.FOREIGN_LEN} and r.n == len(rows) + int(foreign.sum()) > 6 * T.TILE
        assert every_tile_has(foreign) and every_tile_has(~foreign) and no_period_of_a_tile(foreign), name
        assert S.tuples_of(T.select_np(r, own_len), "kmer") == R.parse_rows(rows, S.REDUCE_K)
    assert len(rs) + len(rl) >= S.REDUCE_MIN_ROWS
    for cut in T.UNION_CUTS:
        head = T.key_lengths(inp["short"])[:cut]
        assert 0 < int((head == T.FOREIGN_LEN).sum()) < cut
    big, small = inp["large_long"], inp["large_short"]
    assert big.n == T.LARGE_LONG > 64 * T.TILE and small.n == T.LARGE_SHORT > 2 * T.TILE
    assert set(T.key_lengths(big).tolist()) == {K1, K2} and set(T.key_lengths(small).tolist()) == {K1, K2, T.FOREIGN_LEN}
    for r, own_len in ((big, K2), (small, K1)):
        other = T.key_lengths(r) != own_len
        assert every_tile_has(other) and every_tile_has(~other) and no_period_of_a_tile(other)


def test_the_reduced_set_holds_both_lengths_in_every_tile():
    """the input of rfx_dev_dyn_from_kmers: whichever length a list asks for, every tile of flags has zeros and ones"""
    ln = np.array([len(r[0]) for r in S.reduce_model_run()["st"]["neutral"]])
    assert 100_000 < len(ln) < S.REDUCE_MIN_ROWS and set(ln.tolist()) == {K1, K2}
    assert every_tile_has(ln == K1) and every_tile_has(ln == K2) and no_period_of_a_tile(ln == K1)


# ---- the driver's read set ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_run():
    """the read set at SCALE_G through the parts of reduce_reads_model.model one by one, which keeps every stage of both pairs"""
    reads = T.scale_reads()
    prm = dict(RR.DEFAULTS, P=T.SCALE_P)
    Es = RR.e_rule(T.SCALE_KLIST, prm["min_cov"], prm["min_error_cov"])
    rows, pairs, texts, prev = [], [], [], None
    for i, k in enumerate(T.SCALE_KLIST):
        r, n_mercy = RR.sorter_rows(reads, k, prm)
        assert n_mercy == 0
        rows.append(len(r))
        cur = K.run_text(r, K.default_params(k, max_k=T.SCALE_KLIST[-1], min_error_cov=Es[i])).splitlines(keepends=True)
        if i:
            st, _ = R.run_stages(prev, cur, T.SCALE_KLIST[i - 1], k, T.SCALE_P)
            pairs.append(st)
            texts.append(R.to_text(st["neutral"], T.SCALE_KLIST[i - 1]))
            cur = R.to_text(st["neutral"], k).splitlines(keepends=True)
        prev = cur
    texts.append("".join(prev))
    return dict(reads=reads, Es=Es, rows=rows, pairs=pairs, texts=texts)


def test_the_read_set_is_the_recipe():
    reads = T.scale_reads()
    body, fork = reads[:-22], reads[-22:]
    assert T.SCALE_G % 1000 == 0 and min(map(len, body)) >= 100 and max(map(len, reads)) == 150
    assert sum(T.SCALE_DEPTHS) * T.SCALE_G <= sum(map(len, body)) < sum(T.SCALE_DEPTHS) * T.SCALE_G + 300
    assert len(set(fork[:12])) == 1 and len(set(fork[12:19])) == 1 and sum(a != b for a, b in zip(fork[0], fork[12])) == 1
    assert all(r[18:132] == fork[12][RR.FORK_TAIL:] for r in fork[19:]) and reads == T.scale_reads()


def test_the_driver_input_meets_every_condition_at_the_chosen_size(driver_run):
    d = driver_run
    reads, klist = d["reads"], T.SCALE_KLIST
    info = {}
    assert RR.model(reads, klist, info=info, P=T.SCALE_P) == d["texts"]                  # (the parts above ARE the model's)
    assert info["rows"] == d["rows"] and info["Es"] == d["Es"] == [8, 8, 6]
    caps = [RR.first_capacity(len(reads), max(map(len, reads)), k, 2) for k in klist]
    unions = [len(st["union"]) for st in d["pairs"]]
    print("G", T.SCALE_G, "reads", len(reads), "counter rows", d["rows"], "first capacities", caps, "unions", unions)
    assert min(d["rows"]) >= T.TILE + 1                                                    # the scans and sorts leave one tile at every k
    assert all(n > c for n, c in zip(d["rows"], caps)), (d["rows"], caps)                   # rr_sorted's second count runs at every k
    assert min(unions) >= 65_793, unions                                                   # a block past k_rd_scan_aggs' two aggregates a thread
    for (ka, kb), st in zip(zip(klist, klist[1:]), d["pairs"]):
        for right, name in ((False, "left_sort"), (True, "right_sort")):
            ahead, _ = S.pending_trace(st[name], right, ka)
            print((ka, kb), name, len(ahead), "pending 0/1/2 at the block starts, changes, block starts:", S.state_variety(ahead))
            assert S.variety_holds(ahead), ((ka, kb), name, S.state_variety(ahead))
        assert {len(r[0]) for r in st["neutral"]} == {ka, kb}                              # the pair's final set holds both lengths
    assert sum(t.count("\n") for t in d["texts"]) > T.DEV_FIRST_CAP                        # the caller's first set is short


def test_the_later_k_needs_its_own_e(driver_run):
    """with E = 8 throughout, Count_67_reduced is another text: a driver that kept the first k's E fails the GPU test"""
    wrong = RR.model(driver_run["reads"], T.SCALE_KLIST, Es=[8, 8, 8], P=T.SCALE_P)
    assert wrong[:2] == driver_run["texts"][:2] and wrong[2] != driver_run["texts"][2]
