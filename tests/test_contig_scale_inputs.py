"""The inputs and the fast checkers of tests/test_gpu_contig_scale.py, on the CPU: every numpy / dict statement against the string
model it restates, on inputs the model can do, and every generator against the conditions its test relies on at the seed and size the
GPU test uses (with the 256 CUs of an MI355X where a size depends on the device).  Needs no GPU."""
import numpy as np

from tests import endext_model as E
from tests import extend_model as X
from tests import fixing2_model as F2
from tests import map_model as MP
from tests import mercy_model as MC
from tests import test_gpu_contig_scale as T
from tests.test_gpu_dynamic_packed import words_of
from tests.test_gpu_fixing import value_of, rand_seq
from tests.test_gpu_map import pack_reads

CUS = T.MI355X_CUS
TILE = T.TILE


# ---- the fast checkers against what they restate -----------------------------------------------------------------------------------------
def test_the_numpy_contig_packer_is_the_loop_packer():
    rng = np.random.default_rng(1)
    seqs = [rand_seq(rng, L) for L in [0, 1, 31, 32, 33, 63, 64, 65, 0, 96, 400, 1000] + [int(x) for x in rng.integers(1, 200, 300)]]
    words, woff, ln = T.contig_words_np(seqs)
    loop = [words_of(np.array([T.CODE[ord(ch)] for ch in s], np.uint64)) for s in seqs]
    assert np.array_equal(words, np.concatenate(loop)) and woff.tolist() == [0] + list(np.cumsum([len(w) for w in loop])) and ln.tolist() == [len(s) for s in seqs]
    assert T.contig_words_np([])[0].shape == (0,)
    kmers = [rand_seq(rng, 31) for _ in range(200)] + ["A" * 31, "T" * 31]
    assert T.kmer_values_np(kmers).tolist() == [value_of(k) for k in kmers] and len(T.kmer_values_np([])) == 0


def test_the_read_store_packer_is_pack_reads():
    rng = np.random.default_rng(2)
    lens = np.array([0, 1, 31, 32, 33, 63, 64, 40, 17] + [int(x) for x in rng.integers(0, 65, 100)])
    codes = rng.integers(0, 4, (len(lens), 64), dtype=np.uint8)
    reads = [s[:m] for s, m in zip(T.strings_of(codes.reshape(-1), np.arange(len(lens) + 1) * 64), lens.tolist())]
    for wpr in (2, 3):
        want_w, want_n, _ = pack_reads(reads, wpr)
        got_w, got_n = T.pack_codes(codes, lens, wpr)
        assert np.array_equal(got_w, want_w) and np.array_equal(got_n, want_n)
        junk_w, _ = T.pack_codes(codes, lens, wpr, junk=np.random.default_rng(3))
        as_bits = lambda w: np.unpackbits(w.astype(">u8").view(np.uint8).reshape(len(lens), -1), axis=1)      # noqa: E731
        bits = as_bits(junk_w) != as_bits(want_w)
        assert not (bits & (np.arange(64 * wpr) < 2 * lens[:, None])).any() and bits.sum() > 1000      # the bases are the read's, behind them junk


def special_contigs(rng):
    """the shapes of test_shared_seeds_palindromes_two_ends_in_one_read_and_tandem_repeats (tests/test_gpu_map.py)"""
    pal = "ACGTAGGCTA" + MP.revcomp("ACGTAGGCTA")
    shared, unit = MP.rand_seq(rng, 100), MP.rand_seq(rng, 25)
    cs = [pal + MP.rand_seq(rng, 60), MP.rand_seq(rng, 60) + pal, shared + MP.rand_seq(rng, 50), shared + MP.rand_seq(rng, 400), shared[:40] + MP.rand_seq(rng, 90),
          MP.rand_seq(rng, 450), MP.rand_seq(rng, 450), unit + unit + MP.rand_seq(rng, 40), MP.rand_seq(rng, 20), MP.rand_seq(rng, 21)]
    cs = [(f"Contig_{len(b)}_{i}_{-i}_{i}", b) for i, b in enumerate(cs)]
    reads = ["GG" + cs[0][1][:60], cs[1][1][20:] + "TT", MP.rand_seq(rng, 30) + shared[:70], MP.rand_seq(rng, 9) + shared[:35], cs[5][1][-50:] + cs[6][1][:50],
             "C" + unit * 3, "C" + unit * 4, "A", "ACGTN" * 8, MP.rand_seq(rng, 3) + cs[9][1] + "n"]
    return cs, [x for r in reads for x in (r, MP.revcomp(MP.norm(r)))]


def test_the_indexed_hits_are_the_models():
    """shared seeds, palindromes, two ends in one read, tandem repeats, N; the planted genome; the generators' own shapes at 300 contigs"""
    cs, reads = special_contigs(np.random.default_rng(4))
    for prm in (dict(), dict(seed=20), dict(seed=20, max_mismatch=31), dict(min_overlap=21)):
        hs = MP.hits(cs, reads, **{**MP.DEFAULTS, **prm})
        assert T.hits_indexed(cs, reads, **{**MP.DEFAULTS, **prm}) == hs and len(hs) >= 10, prm
    _, _, cs, reads = MP.planted_case(step=9)
    assert T.hits_indexed(cs, reads) == MP.hits(cs, reads) and len(MP.hits(cs, reads)) > 50
    cs = T.map_contigs(300)
    reads = T.map_reads(cs)[:400]
    hs = MP.hits(cs, reads)
    assert T.hits_indexed(cs, reads) == hs and len(hs) > 300


def test_the_prefiltered_hits_are_the_models():
    """3,073 reads of the grid-cap generator (as if on 2 CUs) through map_model.hits whole"""
    cs, codes, planted = T.grid_cap_reads(2, 513)
    reads = T.strings_of(codes.reshape(-1), np.arange(len(codes) + 1) * T.MAP_READ)
    hs = MP.hits(cs, reads)
    assert T.hits_prefiltered(cs, codes) == hs and {h[0] for h in hs} >= set(planted) and {h[2] for h in hs} == {0, 1} and {h[1] for h in hs} == set(range(6))


def test_the_numpy_mercy_kmers_are_the_models():
    """reads of 16..31 bases from the generator at every k it is used with, and reads of up to 64 bases with clips, poly-A fronts and
    window counts on both sides of the gap rule"""
    for n, k in ((3000, 8), (3000, 11), (3000, 12), (3000, 13), (3000, 15)):
        codes, lens, solid = T.mercy_reads(n, k)
        reads = [s[:m] for s, m in zip(T.strings_of(codes.reshape(-1), np.arange(n + 1) * 32), lens.tolist())]
        kmers = MC.mercy_kmers(reads, k, 0, 0, set(T.kmer_strings(solid, k)))
        keys, per_read = T.mercy_np(codes, lens, k, solid)
        assert np.array_equal(keys, T.mercy_keys_of(kmers)) and len(kmers) > n
        assert per_read.tolist() == [len(MC.mercy_kmers([r], k, 0, 0, set(T.kmer_strings(solid, k)))) for r in reads[:200]] + per_read[200:].tolist()
        assert T.mercy_text_np(keys, k) == "".join(f"{s},1\n" for s in kmers)
    rng = np.random.default_rng(5)
    n, k = 1500, 9
    lens = rng.integers(0, 65, n)
    codes = rng.integers(0, 4, (n, 64), dtype=np.uint8)
    codes[::7, :31] = 0                                             # 31 A in front: nothing from 32 bases on
    codes[np.arange(64) >= lens[:, None]] = 0
    fw, rc = T.window_keys(codes, k)
    solid = np.unique(np.minimum(fw, rc)[:, ::5])[::3]
    reads = [s[:m] for s, m in zip(T.strings_of(codes.reshape(-1), np.arange(n + 1) * 64), lens.tolist())]
    for fc, ec in ((0, 0), (3, 4), (0, 40), (70, 0)):
        kmers = MC.mercy_kmers(reads, k, fc, ec, set(T.kmer_strings(solid, k)))
        assert np.array_equal(T.mercy_np(codes, lens, k, solid, fc, ec)[0], T.mercy_keys_of(kmers)) and (len(kmers) > 1000 or fc + ec >= 40), (fc, ec)
    assert len(T.mercy_np(codes, lens, k, np.zeros(0, np.uint64))[0]) == 0


def test_the_spliced_set_from_a_given_consensus_is_the_models():
    for n, crowded, mk in ((300, 0, T.ENDEXT_MAX_K), (300, 70, 31), (40, 0, 50)):
        contigs, rows = T.endext_input(n, crowded)
        cons = E.device_consensus(contigs, rows)
        recs = T.device_set_from(contigs, cons, mk)
        assert recs == E.device_set(contigs, rows, mk) and (0 < len(recs) < n - 2 or mk == 31)
        assert {r["flags"] for r in recs} >= {0, 1, 2} or n == 40


# ---- A. 05FixingAgain / 06ContigEnds -----------------------------------------------------------------------------------------------------------
def test_the_fix2_records_drop_a_third_in_every_tile():
    assert T.FIX2_SIZES == (4096, 4097, 8193, 270_000) and T.FIX2_SIZES[-1] > T.LANE_WINDOW
    for n in T.FIX2_SIZES:
        r = T.fix2_records(n)
        L = np.diff(r.ext_off[:n + 1]) + np.diff(r.key_off[:n + 1])
        keep = L >= 2 * T.FIX2_MAX_K
        assert r.n == n and set(np.diff(r.key_off[:n + 1]).tolist()) == {F2.KEY} and set(r.marker.tolist()) == {1, 2}
        assert T.every_tile_has(~keep) and T.every_tile_has(keep) and keep[n - 1] and 0.25 < 1 - keep.mean() < 0.4, n
        assert len({t.tobytes() for t in T.tiles(keep) if len(t) == TILE}) == n // TILE                 # no tile repeats another's flags
        assert set(r.left.tolist()) == set(T.MARK.tolist()) == set(r.right.tolist())
        if n < 20_000:
            continue
        cs = T.fix2_model(r)[0]
        two = np.array([len(c[0]) >= 2 * F2.END for c in cs])
        assert len(cs) > 10_000 and len(cs) == int(keep.sum())                                          # idx runs 9,999 -> 10,000
        for edge in (TILE, 2 * TILE, T.LANE_WINDOW // 2):                                               # both record shapes on either side of an edge of toff
            assert two[edge - 200:edge].any() and (~two[edge - 200:edge]).any() and two[edge:edge + 200].any() and (~two[edge:edge + 200]).any()


def test_the_fix2_chain_merges_and_stays_above_a_tile():
    n, mk, P = T.FIX2_CHAIN
    rows = T.fix2_chain_rows()
    last, text, ends = T.fix2_chain_want()
    assert len(rows) == n > TILE and TILE < len(last) < n and text.count("\n") == len(F2.contigs(last, dict(max_k=mk))) > TILE
    assert F2.loop_rounds(F2.default_params(mk, max_iteration=1)) == 2 and {len(r[0]) for r in F2.binarize(rows)} == {F2.KEY}


# ---- B. 07EndExtend ----------------------------------------------------------------------------------------------------------------------------
def key_bits(n):
    bits = 1
    while (1 << bits) <= n:
        bits += 1
    return bits


def test_the_endext_inputs_cross_the_key_width_and_mix_kept_and_dropped_in_string_order():
    assert T.ENDEXT_COUNTS == (4095, 4096, 4097) and [key_bits(n) for n in T.ENDEXT_COUNTS] == [12, 13, 13]
    for n in T.ENDEXT_COUNTS:
        contigs, rows = T.endext_input(n)
        ids = {c[0] for c in contigs}
        named = [E.name_parts(r.split("\t")[0])[0] for r in rows]
        per = np.bincount([int(x.split("_")[4]) for x in named if x in ids], minlength=n)
        assert len(contigs) == n and sum(x not in ids for x in named) == 4 and len(rows) > T.SORT_SMALL and per.max() <= 8 and (per == 0).sum() > n // 5
        assert [len(c[1]) for c in contigs[:2]] == [1, 0]
    # the 4,097 case: the order of the strings is not the order of the numbers, and along it kept and dropped contigs alternate
    cons = E.device_consensus(contigs, rows)
    order = sorted(range(n), key=lambda j: contigs[j][0])
    numeric = sorted(range(n), key=lambda j: tuple(int(x) for x in contigs[j][0].split("_")[1:]))
    assert order != list(range(n)) and order != numeric and order[0] == 1                                # "Contig_0_..." first, "Contig_100_" ahead of "Contig_62_"
    recs = T.device_set_from(contigs, cons, T.ENDEXT_MAX_K)
    kept_src = {r["src_idx"] for r in recs}
    keep = np.array([j in kept_src for j in order])                                                      # by position in the sorted order
    present = np.array([len(contigs[j][1]) >= 2 for j in order])
    assert [r["src_idx"] for r in recs] == [j for j, k in zip(order, keep) if k]
    assert [r["new_idx"] for r in recs] == (np.cumsum(present) - 1)[keep].tolist() and not present[0] and not present.all()
    runs = int((keep[1:] != keep[:-1]).sum())
    assert runs > n // 4 and keep[TILE - 64:TILE].any() and (~keep[TILE - 64:TILE]).any() and keep[TILE], (runs, keep[TILE - 8:].tolist())
    assert {r["flags"] for r in recs} == {0, 1, 2, 3} and any(len(w[0]) and len(w[1]) for w in cons)


def test_the_endext_sort_cases_take_the_top_digit_path_and_leave_it():
    for case, (n, crowded) in T.ENDEXT_SORT_CASES.items():
        contigs, rows = T.endext_input(n, crowded, pairs=9)
        ids = {c[0]: i for i, c in enumerate(contigs)}
        keys = np.array([ids.get(E.name_parts(r.split("\t")[0])[0], n) for r in rows])
        buckets = np.bincount(keys >> (key_bits(n) - 8))
        assert n > 255 and key_bits(n) > 8 and len(rows) > T.SORT_SMALL and len(rows) <= 192 * T.SORT_SMALL
        assert (buckets.max() > T.SORT_SMALL) == (crowded > 0) and (np.bincount(keys).max() > T.SORT_SMALL) == (crowded > 0), (case, buckets.max())


# ---- C. 08Extend / 09ExtendAgain ---------------------------------------------------------------------------------------------------------------
def test_the_ext_rows_drop_rows_in_every_tile_and_their_three_offsets_cross_a_tile_apart():
    for n in T.EXT_ROWS:
        rows = T.ext_rows(n)
        p = X.default_params(T.EXT_MAX_K, max_iteration=0)
        kept, k, w = T.ext_offsets(rows, p)
        longs, kmers = X.contig_ends(X.binarize(rows, p), p)
        assert int(kept.sum()) == len(longs) and int(k.sum()) == len(kmers) and int(w.sum()) == sum((len(r[2]) + 31) // 32 for r in longs)
        assert T.every_tile_has(~kept) and T.every_tile_has(kept) and 0.05 < 1 - kept.mean() < 0.3
        cross = [int(np.searchsorted(np.cumsum(a), TILE, side="right")) for a in (k, kept.astype(int), w)]      # the contig where each reaches 4,096
        assert len(set(cross)) == 3 and max(cross[0], cross[2]) < n and (cross[1] < n or n < 2 * TILE), cross
        dev = X.device_set(rows, p, True)
        flags = np.array([c["flags"] for c in dev])
        pos = np.cumsum(kept) - 1                                                                            # a row's place among the kept
        for c in cross + [TILE]:
            if c + 8 < n:
                q = int(pos[c])
                assert set(flags[q - 8:q].tolist()) == {0, 1, 2, 3} == set(flags[q:q + 8].tolist()), (n, c)
        assert {c["flags"] for c in X.device_set(rows, p, False)} == {0}
        assert X.seam_overlaps(dev, p) == {(s, m) for s in "LR" for m in (1, 2, 3)}


def test_the_ext_chain_stays_above_a_tile_through_both_stages():
    n, mk, P, it = T.EXT_CHAIN
    rows = T.ext_chain_rows()
    last, text, cs, text2 = T.ext_chain_want()
    p = X.default_params(mk, max_iteration=it)
    assert len(rows) == n > TILE and len(X.binarize(rows, p)) == n and len(last) > TILE and TILE < len(cs) <= n
    assert sum(c["flags"] != 0 for c in X.device_set(rows, p, True)) > n // 4 and text2.count("\n") == len(cs)


# ---- D. the end mapper -------------------------------------------------------------------------------------------------------------------------
def test_the_map_inputs_put_the_seed_table_on_each_sort_path():
    assert [4 * n for n in T.MAP_CONTIG_COUNTS] == [T.SORT_SMALL, T.SORT_SMALL + 4, T.SORT_TWO_LEVELS + 4]
    for n in T.MAP_CONTIG_COUNTS:
        contigs = T.map_contigs(n)
        reads = T.map_reads(contigs)
        hs = T.hits_indexed(contigs, reads)
        ends = np.array(sorted({h[1] for h in hs}))
        assert len(contigs) == n and all(62 <= len(b) <= 140 for _, b in contigs) and 2 * min(T.MAP_PLANTED, n) + 200 <= len(reads) < 5000
        assert {0, 1, 2 * n - 2, 2 * n - 1} <= set(ends.tolist()) and all(((ends >= 2 * n * q // 8) & (ends < 2 * n * (q + 1) // 8)).sum() > 20 for q in range(8))
        assert {h[2] for h in hs} == {0, 1} and len({h[0] for h in hs}) >= (len(reads) - 200) * 9 // 10
        table = T.seed_table(MP.ends_of(contigs), T.MAP_SEED)
        shared = [v for v in table.values() if len(v) > 1]
        far = [v for v in shared if abs(v[0] - v[-1]) >= n // 2]
        by_read = {}
        for h in hs:
            by_read.setdefault((h[0], h[2]), set()).add(h[1])
        assert len(far) >= min(T.MAP_SHARED, n // 4) * 9 // 10 and any(len(v) > 1 and max(v) - min(v) >= n // 2 for v in by_read.values())


def test_the_grid_cap_reads_put_rows_in_the_last_reads_and_in_the_second_trip():
    cap = 5 * CUS * 256
    assert cap == 327_680 > T.LANE_WINDOW
    for extra in (0, 1, 257):
        contigs, codes, planted = T.grid_cap_reads(CUS, extra)
        with_rows = {h[0] for h in T.hits_prefiltered(contigs, codes)}
        n = len(codes)
        assert n == cap + extra and codes.shape[1] == T.MAP_READ and set(planted) <= with_rows and len(with_rows) < 1000
        assert sum(i >= n - 300 for i in with_rows) >= 90 and min(with_rows) < 1000
        if extra:
            assert cap in with_rows and n - 1 in with_rows                                           # the first block's second trip
        if extra == 257:
            assert sum(cap <= i < cap + 256 for i in with_rows) > 150 and cap + 256 in with_rows     # ... and the second block's


# ---- E. the mercy stage ------------------------------------------------------------------------------------------------------------------------
def test_the_mercy_reads_leave_zeros_in_every_tile_and_k_mers_on_the_second_trip():
    cap = T.MERCY_WAVES_PER_CU * CUS
    sizes = T.mercy_sizes(CUS)
    assert [n for n, _ in sizes] == [4096, 4097, 8192, 8193] and cap == 8192 and T.MERCY_LARGE > T.LANE_WINDOW
    for n, k in sizes + [(T.MERCY_LARGE, T.MERCY_K[T.MERCY_LARGE])]:
        codes, lens, solid = T.mercy_reads(n, k)
        keys, per_read = T.mercy_np(codes, lens, k, solid)
        assert 8 <= k <= 15 and lens.max() <= 31 and np.array_equal(solid, np.unique(solid))
        assert 0.3 < (per_read == 0).mean() < 0.55 and T.every_tile_has(per_read == 0) and T.every_tile_has(per_read > 0) and per_read[n - 1] > 0, (n, k)
        assert (lens == 16).mean() > 0.3 and len(keys) > n
        if n > cap:                                                 # reads of the second trip: some give k-mers, some (but at 8,193) are skipped
            assert per_read[cap:].any() and (n == cap + 1 or (per_read[cap:] == 0).any()) and (per_read[:cap] == 0).any()


def test_the_mercy_count_rows_are_past_the_two_level_threshold_with_repeats_and_foreign_rows():
    distinct, repeats, foreign, k = T.MERCY_ROWS
    rows, reads = T.mercy_count_rows()
    ln = np.array([len(r.split(",")[0]) for r in rows])
    own = [r.split(",")[0] for r in rows if len(r.split(",")[0]) == k]
    assert len(rows) == distinct + repeats + foreign and len(own) == distinct + repeats > T.SORT_TWO_LEVELS
    assert T.every_tile_has(ln != k) and T.every_tile_has(ln == k) and set(ln.tolist()) == {k - 1, k, k + 1}
    solid = MC.solid_set(rows, k)
    assert len(solid) == len(set(own)) and distinct - 100 < len(solid) <= distinct
    assert len(reads) == T.MERCY_ROW_READS and len(MC.mercy_kmers(reads, k, 0, 0, solid)) > T.MERCY_ROW_READS
