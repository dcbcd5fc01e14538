"""The inputs and the fast checkers of tests/test_gpu_dedup_scale.py, on the CPU: every generator against the conditions its test
relies on at the seed and size the GPU test uses (the fourth table), counted on the generator's plan and on
oracle.dedup_contigs alone, and the list forms of the layout and the two texts against the statements they restate.  Needs no GPU."""
import functools

import numpy as np

from oracle import oracle as O
from tests import test_gpu_dedup_packed as P
from tests import test_gpu_dedup_scale as T
from tests.test_gpu_contig_scale import every_tile_has

TILE = T.TILE
MARKER_LIMIT = 1 << 26                                              # sort_pairs takes a third MSD level from here on: not reached


# ---- rfx_dedup.hip's counts of marker rows, restated ------------------------------------------------------------------------------------
def seed_count(L):
    """dd_seed_count: a seed at every block start 0, 31, 62, .. of a contig of at least 300 bases that a whole 31-mer follows"""
    return 0 if L < 300 else (L - 1) // 31 + (1 if L % 31 == 0 else 0)


def probe_windows(L):
    """dd_windows: the [a, b) of probe positions"""
    M = 31
    if L >= 2000:
        side = 1000 if L >= 4000 else 600
        return [(0, M), (side - M + 1, side), ((L - 2 * M) // 2, (L - 2 * M) // 2 + M), (L - side - M + 1, L - side), (L - 2 * M, L - M)]
    return [(0, M), ((L - 2 * M) // 3, (L - 2 * M) // 3 + M), ((L - 2 * M) * 2 // 3, (L - 2 * M) * 2 // 3 + M), (L - 2 * M, L - M)]


def probe_positions(L):
    """dd_probe_positions"""
    return 0 if L < 300 else sum(b - a for a, b in probe_windows(L))


def marker_rows(contigs, rnd):
    """the rows k_dd_markers writes in round rnd: the seeds and the probes, both strands of a probe from round 2 on"""
    return sum(seed_count(len(s)) + probe_positions(len(s)) * (2 if rnd > 1 else 1) for s in contigs)


def seeds_inside(a, b):
    """the 15-mer seeds of a long contig (at 0, 15, 30, ..) that lie wholly in [a, b): each is one entry of the distance list of a
    short contig that covers [a, b)"""
    return max(0, (b - 15) // 15 - -(-a // 15) + 1)


@functools.lru_cache(maxsize=None)
def made(which):
    contigs, plan = T.round_set(**T.ROUND_SETS[which])
    return contigs, plan, O.dedup_contigs(contigs)


def leftover(final):
    return sum(1 for s in final if s.startswith("T" * 31) and len(s) <= 62)


# ---- the sets of the three rounds ---------------------------------------------------------------------------------------------------------
def test_the_marker_sorts_lie_on_the_paths_the_tests_name():
    assert (T.SORT_SMALL, T.SORT_TWO_LEVELS) == (2048, 393_216)
    assert probe_positions(700) == 124 and probe_positions(2000) == probe_positions(150_000) == 153 and probe_positions(299) == 0
    assert (seed_count(299), seed_count(300), seed_count(310), seed_count(311)) == (0, 9, 10, 10)
    m = {which: (marker_rows(made(which)[0], 1), marker_rows(made(which)[0], 2)) for which in T.ROUND_SETS}
    assert T.SORT_SMALL < m[1][0] <= T.SORT_TWO_LEVELS < m[1][1]           # set 1 straddles the two-level threshold
    for which in (2, 3, 4):
        assert T.SORT_TWO_LEVELS < m[which][0] < m[which][1] < MARKER_LIMIT, which
    assert m == T.MARKER_ROWS


def test_step_0_batches_more_than_1024_merges_and_its_distance_list_leaves_the_small_sort():
    """counted on the plan: the groups with a reverse-complemented short contig (merged in round 1) and with a forward one (round
    2), and the entries of round 1's step-0 distance list -- one for every seed of the long contig that lies wholly under the short
    one, so about a fifteenth of the overlap"""
    groups = {which: made(which)[1] for which in T.ROUND_SETS}
    with_rc = {which: sum(1 for _, sh in g if any(s == "rc" for s, _, _ in sh)) for which, g in groups.items()}
    with_fwd = {which: sum(1 for _, sh in g if any(s == "fwd" for s, _, _ in sh)) for which, g in groups.items()}
    assert with_rc[2] >= 1_025 and with_rc[3] >= 4_097 and with_fwd[3] >= 1_025
    assert with_fwd[2] == 2 * 275              # two kinds in eight bring a forward piece: set 2's round 2 stays below 1,025 merges a step, set 3's does not
    for which, first, second in ((2, with_rc[2], with_fwd[2]), (3, with_rc[3], with_fwd[3])):
        n, rounds = len(made(which)[0]), [len(r) for r in made(which)[2]["rounds"]]
        assert n - rounds[0] >= first and rounds[0] - rounds[1] >= second, which
    # the query threads of step 0 (every 15-mer of the first short of a group) and the list's entries
    queries = {which: sum(min(b - a for s, a, b in sh if s == "rc") - 14 for _, sh in g if any(s == "rc" for s, _, _ in sh)) for which, g in groups.items()}
    entries = {which: sum(min(seeds_inside(a, b) for s, a, b in sh if s == "rc") for _, sh in g if any(s == "rc" for s, _, _ in sh)) for which, g in groups.items()}
    assert queries[2] > T.SORT_TWO_LEVELS
    assert T.SORT_SMALL < entries[1] < entries[2] < entries[3] <= T.SORT_TWO_LEVELS < entries[4]
    assert entries == T.STEP0_ENTRIES
    # one list of the long pair: a run of equal distances that the 64-ary search of k_dd_vote takes in three levels, resp. four
    assert 64 ** 2 < seeds_inside(0, T.LONG_PAIR) <= 64 ** 3 < T.SORT_TWO_LEVELS < seeds_inside(0, T.LONGER_PAIR) <= 64 ** 4
    # key_bits = 33 + ceil(log2 nm): the merges of round 1's step 0 need 10, 11 and 13 bits above the distance
    assert [int(np.ceil(np.log2(with_rc[w]))) for w in (1, 2, 3)] == [10, 11, 13]


def test_groups_of_one_two_three_and_120_shorts():
    for which in (1, 2, 3):
        per_group = {len(sh) for _, sh in made(which)[1]}
        assert per_group >= {1, 2, 3}, which
    hub = [sh for L, sh in made(2)[1] if L == T.HUB[0]]
    assert len(hub) == 1 and len(hub[0]) == T.HUB[1] == 120 < 155      # below what section 16 allows a contig in candidate pairs
    assert all(b - a == T.HUB[2] >= 300 for _, a, b in hub[0])


def test_marker_rows_are_left_over_and_the_oracle_gives_what_the_gpu_file_stores():
    for which in T.ROUND_SETS:
        contigs, _, w = made(which)
        got = dict(n=len(contigs), rounds=[len(r) for r in w["rounds"]], candidates=w["candidates"], leftover=leftover(w["rounds"][2]))
        assert got == T.EXPECT[which], (which, got)
        assert got["leftover"] > 0, which
    # with rows left over the bound "the input's sizes suffice" of the capacity contract does not come from the merges alone
    contigs, _, w = made(2)
    assert len(w["rounds"][2]) < len(contigs)


def test_the_shuffle_spreads_the_groups_over_the_tiles_of_contigs():
    """set 2 and set 3 hold more than one look-back tile of contigs, and contigs that probe (300 bases and up) and contigs that do
    not lie in every full tile"""
    for which in (2, 3):
        ln = np.array([len(s) for s in made(which)[0]])
        assert len(ln) > TILE and every_tile_has(ln >= 300) and every_tile_has(ln < 300) and every_tile_has(ln == 0), which


# ---- the skewed set -------------------------------------------------------------------------------------------------------------------------
def mers31(s):
    """the 31-mers of s at every position, as integers"""
    c = P.CODE[np.frombuffer(s.encode(), np.uint8)]
    w = np.lib.stride_tricks.sliding_window_view(c, 31)
    return (w << (np.uint64(2) * np.arange(30, -1, -1, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


def test_the_skewed_set_makes_runs_of_equal_keys_longer_than_a_sort_tile():
    contigs, S = T.skew_set()
    copies, L, strangers, _ = T.SKEW
    assert len(contigs) == 2 * copies + strangers and contigs.count(S) == copies == contigs.count(P.rc(S))
    # round 1's rows of one copy of S and of one of rc(S): the seeds as they read, the probes reverse-complemented
    rows = []
    for s in (S, P.rc(S)):
        fw, bw = mers31(s), mers31(P.rc(s))
        rows.append(fw[31 * np.arange(seed_count(L))])
        rows.append(np.concatenate([bw[L - 31 - np.arange(a, b)] for a, b in probe_windows(L)]))
    keys, counts = np.unique(np.concatenate(rows), return_counts=True)
    shared = counts[counts >= 2]
    assert len(shared) >= 4                                          # seed 31-mers of one strand under a probe window of the other
    assert int(shared.min()) * copies == 2 * copies > T.SORT_SMALL == 8 * 256      # a run of 2,060 rows: a sort tile, eight blocks of k_dd_select
    m1 = marker_rows(contigs, 1)
    assert T.SORT_SMALL < m1 <= T.SORT_TWO_LEVELS                    # the top-digit path, whose buckets of 2,060 equal keys end in the LSD passes
    w = O.dedup_contigs(contigs)
    got = dict(n=len(contigs), rounds=[len(r) for r in w["rounds"]], candidates=w["candidates"], leftover=leftover(w["rounds"][2]))
    assert got == T.EXPECT["skew"], got
    assert w["candidates"][0] > 1_024 and w["candidates"][1] > 1_024 and w["candidates"][2] == 0     # one group of that many shorts: a step a short
    assert got["rounds"] == [copies + strangers, strangers + 1, strangers + 1]


# ---- the layout inputs ----------------------------------------------------------------------------------------------------------------------
def every_scan_tile_has(flags):
    """every full tile of 2,048 (exclusive_scan_u64's) holds a set flag, and so every one of 4,096"""
    return all(flags[i:i + T.SCAN_TILE].any() for i in range(0, len(flags) - T.SCAN_TILE + 1, T.SCAN_TILE))


def test_every_tile_of_the_layout_inputs_drops_and_keeps_contigs():
    assert T.LAYOUT_SIZES == (2048, 2049, 4095, 4096, 4097, 8193) and T.LAYOUT_BIG > T.LANE_WINDOW == 64 * TILE and TILE == 2 * T.SCAN_TILE
    for n in T.LAYOUT_SIZES + (T.LAYOUT_BIG,):
        contigs = T.layout_contigs(n)
        ln = np.array([len(s) for s in contigs])
        assert len(ln) == n and every_scan_tile_has(ln == 0) and every_tile_has(ln == 0), n
        for min_contig in T.MIN_CONTIGS[1:] if n < T.LAYOUT_BIG else T.MIN_CONTIGS[1:2]:
            assert every_scan_tile_has((ln > 0) & (ln < min_contig)) and every_scan_tile_has(ln >= min_contig), (n, min_contig)
        assert ln[n - 1] >= max(T.MIN_CONTIGS) or n == T.LAYOUT_BIG  # the tile of one element (2,049, 4,097, 8,193) is kept
        text = "".join(contigs)
        assert "N" in text and "a" in text and "n" in text
        assert (set(ln.tolist()) == set(P.LENGTHS)) if n < T.LAYOUT_BIG else (ln.min() == 0 and ln.max() == T.LAYOUT_BIG_MAX and 9_000_000 < ln.sum() < 10_000_000)


def test_the_header_grows_a_column_between_kept_contigs():
    ln = np.array([len(s) for s in T.layout_contigs(T.LAYOUT_BIG)])
    assert T.KEPT_AT == (9_999, 10_000, 99_999, 100_000) and (ln[list(T.KEPT_AT)] >= 32).all()
    assert [len(h) for h in T.headers_of(ln[list(T.KEPT_AT)], np.array(T.KEPT_AT))] == [15, 16, 16, 17]


# ---- the fast checkers against what they restate ----------------------------------------------------------------------------------------------
def test_the_list_forms_are_the_statements_of_the_existing_file():
    rng = np.random.default_rng(3)
    alphabet = np.frombuffer(b"ACGTACGTACGTNacgtn", np.uint8)
    lens = [0, 0, 1, 31, 32, 33, 63, 64, 65, 99, 100, 0] + [int(x) for x in rng.integers(0, 101, 400)] + [0]
    short = [alphabet[rng.integers(0, len(alphabet), L)].tobytes().decode() for L in lens]
    mixed = P.mixed_contigs(rng, 300) + [""]
    for contigs in (short, mixed, [], [""]):
        words, woff, ln = T.contig_words_np(contigs)
        loop = [P.words_of(s) for s in contigs]
        assert np.array_equal(words, np.concatenate(loop) if loop else np.zeros(0, np.uint64))
        assert woff.tolist() == [0] + np.cumsum([len(w) for w in loop]).tolist() and ln.tolist() == [len(s) for s in contigs]
        assert T.as_t_fast(contigs) == [P.as_t(s) for s in contigs]
        for min_contig in (0, 1, 32, 64, 500):
            assert T.text_of_fast(contigs, min_contig) == P.text_of(contigs, min_contig)
    for contigs in (short, [], [""]):
        for eol in ("\n", "\r\n"):
            for junk in (True, False):
                assert T.path_text_fast(contigs, eol, junk) == P.path_text(contigs, eol, junk)
