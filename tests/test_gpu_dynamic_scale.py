"""The packed dynamic-k stages past the sizes where their launches change shape: pack / unpack / text over
more than 1 and more than 64 look-back scan tiles, rfx_dev_dyn_sort's chained sorts on either side of sort_pairs' two-level
threshold, the extend pass over more than one tile, the sorting, reduction and fixing stages with more rows than one thread of a
one-block aggregate scan gets one aggregate for, more contigs than one scan tile, and the 62-bit sort of rfx_dev_fix_kmer_set on
the two-level path.  Every comparison is exact, against the string models (tests/pymodel.py, ksort_model.py, reduce_model.py,
fixing_model.py) or a numpy statement of them that tests/test_scale_inputs.py pins to the model on the CPU; the generators and
the vectorised helpers live here and are checked there too (the conditions each input must meet are conditions on the INPUT).
The record-by-record checkers of the stage files loop in Python; above ~20,000 records this file compares with np_packed_fast."""
import os
from collections import Counter

import numpy as np
import pytest

from tests import fixing_model as F
from tests import ksort_model as K
from tests import pymodel as M
from tests import reduce_model as R
from tests import test_gpu_fixing as TF
from tests import test_gpu_ksort as TK
from tests.test_gpu_dynamic_edges import same_records
from tests.test_gpu_dynamic_packed import records_of, KEY_LENGTHS, EXT_LENGTHS
from tests.test_gpu_ksort import upload
from tests.test_gpu_reduce import crafted_rows, dev_starts, lines

pytestmark = pytest.mark.gpu

NUC = np.frombuffer(b"ACGT", np.uint8)
I64_MIN = np.iinfo(np.int64).min
SORT_TILE = 2048                                                   # rfx_sort.hip: a final bucket above it takes the LSD passes


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


# ---- ragged record sets as numpy arrays -----------------------------------------------------------------------------------------------
def dyn_records(key, key_off, ext, ext_off, marker, left, right):
    from reflexiv_amd.api import DynRecords
    codes = lambda a: np.ascontiguousarray(a, np.uint8) if len(a) else np.zeros(1, np.uint8)      # noqa: E731
    return DynRecords(codes(key), np.ascontiguousarray(key_off, np.int64), codes(ext), np.ascontiguousarray(ext_off, np.int64),
                      np.ascontiguousarray(marker, np.int32), np.ascontiguousarray(left, np.int32), np.ascontiguousarray(right, np.int32))


def offsets_of(lengths):
    off = np.zeros(len(lengths) + 1, np.int64)
    off[1:] = np.cumsum(lengths)
    return off


def segments(off, sel):
    """the segments `sel` of a ragged array with offsets off -> (flat indices of their elements, the new offsets)"""
    new = offsets_of((off[1:] - off[:-1])[sel])
    return np.repeat(off[:-1][sel] - new[:-1], np.diff(new)) + np.arange(new[-1]), new


def take(r, sel):
    """the records sel (an index array) of r, in that order"""
    ki, ko = segments(r.key_off[:r.n + 1], sel)
    ei, eo = segments(r.ext_off[:r.n + 1], sel)
    return dyn_records(r.key[ki], ko, r.ext[ei], eo, r.marker[sel], r.left[sel], r.right[sel])


def concat(a, b):
    ka, ea = int(a.key_off[a.n]), int(a.ext_off[a.n])
    return dyn_records(np.concatenate([a.key[:ka], b.key[:int(b.key_off[b.n])]]), np.concatenate([a.key_off[:a.n], b.key_off[:b.n + 1] + ka]),
                       np.concatenate([a.ext[:ea], b.ext[:int(b.ext_off[b.n])]]), np.concatenate([a.ext_off[:a.n], b.ext_off[:b.n + 1] + ea]),
                       np.concatenate([a.marker, b.marker]), np.concatenate([a.left, b.left]), np.concatenate([a.right, b.right]))


def strings_of(codes, off):
    b = NUC[codes[:int(off[-1])]].tobytes().decode()
    return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def tuples_of(r, form):
    """r as the models' tuples: form "dyn" (key, marker, ext, left, right) or "kmer" (key, ext, marker, left, right)"""
    k, e = strings_of(r.key, r.key_off[:r.n + 1]), strings_of(r.ext, r.ext_off[:r.n + 1])
    mk, lf, rt = r.marker.tolist(), r.left.tolist(), r.right.tolist()
    return list(zip(k, mk, e, lf, rt)) if form == "dyn" else list(zip(k, e, mk, lf, rt))


def host_kmer(recs):
    return TK.host(recs)                                           # (key, ext, marker, left, right)


def host_dyn(recs):
    return TF.host(recs)                                           # (key, marker, ext, left, right)


# ---- the numpy packer, without a loop over the records ---------------------------------------------------------------------------------
def words_of_ragged(codes, off, words_per_record=None):
    """ragged base codes -> 64-bit words, 32 bases each, the first in the two highest bits, 0 behind a record's last base; a record
    takes words_per_record words, or as many as its bases need -> (words, word offsets)"""
    n = len(off) - 1
    ln = off[1:] - off[:-1]
    woff = np.arange(n + 1, dtype=np.int64) * words_per_record if words_per_record else offsets_of((ln + 31) // 32)
    flat = np.zeros(int(woff[-1]) * 32, np.uint8)
    flat[np.repeat(woff[:-1] * 32 - off[:-1], ln) + np.arange(off[0], off[-1])] = codes[off[0]:off[-1]]
    q = flat.reshape(-1, 4)
    b = np.ascontiguousarray((q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3], np.uint8)      # (codes are 0..3: no carry)
    return b.view(">u8").astype(np.uint64), woff


def np_packed_fast(r):
    """np_packed of test_gpu_dynamic_packed.py: (key [n, 4], key_len, ext words, ext_off in words, ext_len)"""
    n = r.n
    ko, eo = r.key_off[:n + 1], r.ext_off[:n + 1]
    key, _ = words_of_ragged(r.key, ko, 4)
    ext, woff = words_of_ragged(r.ext, eo)
    return key.reshape(n, 4), np.diff(ko).astype(np.uint8), ext, woff, np.diff(eo).astype(np.int32)


def raw_equals_fast(pk, r, tag):
    """raw_equals of test_gpu_dynamic_packed.py on the vectorised packer: the words in HBM are the numpy packer's of record set r"""
    key, key_len, ext, ext_off, ext_len, marker, left, right = pk.host()
    wk, wkl, we, weo, wel = np_packed_fast(r)
    for name, a, b in (("key", key, wk), ("key_len", key_len, wkl), ("ext_off", ext_off, weo), ("ext_len", ext_len, wel), ("ext", ext, we),
                       ("marker", marker, r.marker[:r.n]), ("left", left, r.left[:r.n]), ("right", right, r.right[:r.n])):
        if a.shape != b.shape or not np.array_equal(a, b):
            i = int(np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[0]) if a.shape == b.shape else -1
            raise AssertionError((tag, name, a.shape, b.shape, "first difference at", i))


def equals_fast(rfx, pk, want, tag):
    """the packed set in HBM is the record set `want` (a DynRecords): unpacked field by field, and word for word the numpy packer's"""
    same_records(rfx.dyn_unpack(pk), want, tag)
    raw_equals_fast(pk, want, tag)


# ---- a numpy statement of pymodel.dyn_sort's order and of dyn_partition_starts -----------------------------------------------------------
def block_columns(r):
    """pymodel.dyn_blocks for every key: four int64 columns (the signed 31-base blocks, 01 behind the last base; the smallest long
    where the key has no such block) and the block count"""
    n = r.n
    off = r.key_off[:n + 1]
    ln = off[1:] - off[:-1]
    mat = np.zeros((n, 128), np.uint8)
    mat.reshape(-1)[np.repeat(np.arange(n, dtype=np.int64) * 128 - off[:-1], ln) + np.arange(off[0], off[-1])] = r.key[off[0]:off[-1]]
    nb = np.maximum(1, (ln + 30) // 31)
    cols = []
    for j in range(4):
        sub = np.zeros((n, 32), np.uint8)
        sub[:, :31] = mat[:, 31 * j:31 * j + 31]
        q = sub.reshape(n, 8, 4)
        b = np.ascontiguousarray((q[..., 0] << 6) | (q[..., 1] << 4) | (q[..., 2] << 2) | q[..., 3], np.uint8)
        v = b.view(">u8").reshape(n).astype(np.uint64)
        m = np.clip(ln - 31 * j, 0, 31).astype(np.uint64)
        last = (31 * j + 31 >= ln) & (j < nb)
        v = np.where(last, v | (np.uint64(1) << (np.uint64(2) * (np.uint64(31) - m))), v).view(np.int64)
        v[j >= nb] = I64_MIN
        cols.append(v)
    return cols, nb


def sort_order(r):
    """the permutation of pymodel.dyn_sort: tuples of signed blocks element by element, a proper prefix first, stable.  A block the
    key lacks compares as the smallest long, and the block count breaks what is then still a tie (only G A^30 in a block that is
    not the key's last IS the smallest long; the longer key follows, as in the tuple order)"""
    cols, nb = block_columns(r)
    return np.lexsort((nb, cols[3], cols[2], cols[1], cols[0]))


def key_edges(r):
    """the rows of a SORTED set whose key differs from the row before (row 0 among them), and n"""
    cols, nb = block_columns(r)
    k = np.stack(cols + [nb.astype(np.int64)])
    return np.concatenate([[0], 1 + np.flatnonzero((k[:, 1:] != k[:, :-1]).any(axis=0)), [r.n]]) if r.n else np.array([0])


def partition_starts_np(r, P, edges=None):
    """pymodel.dyn_partition_starts on a SORTED set: floor(p n / P), moved forward past equal keys"""
    edges = key_edges(r) if edges is None else edges
    n = r.n
    st, prev = [], 0
    for p in range(P):
        s = max(p * n // P, prev)
        if 0 < s < n:
            s = int(edges[np.searchsorted(edges, s)])
        st.append(s)
        prev = s
    return st + [n]


def top16_histogram_max(r):
    """the largest bin of the 16 highest bits of the first block over the records (the sign bit flipped or not: the same bins)"""
    cols, _ = block_columns(r)
    return int(np.bincount((cols[0].view(np.uint64) >> np.uint64(48)).astype(np.int64), minlength=1 << 16).max())


# ---- a. pack, unpack, text --------------------------------------------------------------------------------------------------------------
PACK_SIZES = (4096, 4097, 8193, 270_000)


def pack_records(n):
    """records_of of test_gpu_dynamic_packed.py; at 270,000 the same classes drawn by numpy, the 1,000-base extension class thinned to
    one record in 50 (the others of that class take the shorter lengths in turn)"""
    rng = np.random.default_rng(60 + n)
    if n < 20_000:
        return records_of(rng, n)
    i = np.arange(n)
    kl, el = np.array(KEY_LENGTHS)[i % 13], np.array(EXT_LENGTHS)[i % 9]
    el = np.where((i % 9 == 8) & ((i // 9) % 50 != 0), np.array(EXT_LENGTHS)[(i // 9) % 8], el)
    ko, eo = offsets_of(kl), offsets_of(el)
    return dyn_records(rng.integers(0, 4, ko[-1], dtype=np.uint8), ko, rng.integers(0, 4, eo[-1], dtype=np.uint8), eo, 1 + i % 2,
                       rng.integers(-50, 50, n), rng.integers(-50, 50, n))


def text_of_records(r):
    return "".join(f"{k},{a},{e}\n" for k, a, e in r.rows()).encode()


@pytest.mark.parametrize("n", PACK_SIZES)
def test_pack_unpack_and_text_over_more_than_one_scan_tile(rfx, n):
    """n = 4096 | 4097 | 8193: one, two and three tiles of the look-back scans (the extension offsets by the single scan, the text's
    key / extension offsets by the dual one); 270,000 = 66 tiles, so a tile has more than the 64 predecessors one lane window
    covers and the look-back's second window is REACHABLE -- whether a tile takes it depends on which tiles have published when it
    looks, which a test cannot force -- and exclusive_scan_u64 runs two levels.  unpack(pack(x)) = x field by field, the raw words
    are the numpy packer's, the text is the host's."""
    r = pack_records(n)
    assert r.n == n and {(int(a), int(b)) for a, b in zip(np.diff(r.key_off), np.diff(r.ext_off))} == {(a, b) for a in KEY_LENGTHS for b in EXT_LENGTHS}
    pk = rfx.dyn_pack(r)
    assert pk.n == n
    raw_equals_fast(pk, r, ("pack", n))
    same_records(rfx.dyn_unpack(pk), r, ("unpack", n))
    d_text, ln = rfx.dyn_to_text_dev(pk)
    want = text_of_records(r)
    assert ln == len(want) and bytes(d_text[:ln].cpu().numpy()) == want, ("text", n)


# ---- b. rfx_dev_dyn_sort on either side of the two-level threshold -------------------------------------------------------------------------
SORT_CASES = ((393_216, False), (400_000, False), (400_000, True))
SORT_DUP_KEYS, SORT_SKEW_KEYS = 2000, 4000
SORT_SKEW_PREFIX = np.array([1, 3, 0, 2, 2, 1, 0, 3], np.uint8)    # CTAGGCAT


def sort_records(n, skewed):
    """n records in random order: keys of 1..124 bases (every block count), 2,000 of the keys of 16 bases or more held by 3 to 6
    records whose extensions differ in length (so a sort that is not stable shows), the others by one record with a one-base
    extension; skewed: 4,000 keys of 9 bases or more begin with the same 8 bases, so one bin of the first block's 16 highest bits
    holds more rows than a sort tile"""
    rng = np.random.default_rng(n + int(skewed))
    copies = rng.integers(3, 7, SORT_DUP_KEYS)
    m = n - int(copies.sum()) + SORT_DUP_KEYS
    kl = rng.integers(1, 125, m)
    ko = offsets_of(kl)
    key = rng.integers(0, 4, ko[-1], dtype=np.uint8)
    if skewed:
        for s in rng.choice(np.flatnonzero(kl >= 9), SORT_SKEW_KEYS, replace=False):
            key[ko[s]:ko[s] + 8] = SORT_SKEW_PREFIX
    rep = np.ones(m, np.int64)
    rep[rng.choice(np.flatnonzero(kl >= 16), SORT_DUP_KEYS, replace=False)] = copies
    slot = np.repeat(np.arange(m), rep)
    copy = np.arange(n) - np.repeat(offsets_of(rep)[:-1], rep)                     # 0 .. 5 within a key's records
    order = rng.permutation(n)
    slot, copy = slot[order], copy[order]
    ki, nko = segments(ko, slot)
    eo = offsets_of(1 + copy)
    return dyn_records(key[ki], nko, rng.integers(0, 4, eo[-1], dtype=np.uint8), eo, rng.integers(1, 3, n), rng.integers(-50, 50, n),
                       rng.integers(-50, 50, n))


@pytest.mark.parametrize("n,skewed", SORT_CASES)
def test_dyn_sort_around_the_two_level_threshold(rfx, n, skewed):
    """393,216 rows are 192 sort tiles, the last size of sort_pairs' top-digit path; 400,000 take two MSD levels.  The keys reach four
    blocks, so the 8-bit count pass and all four block passes run, each carrying the permutation of the one before; a block that
    some keys lack is one oversized bucket, so those passes finish by the LSD passes from the regrouped state, and with the skewed
    keys the first block's pass does too.  Against the numpy statement of pymodel.dyn_sort, the cut for P = 1, 7, 63 included."""
    r = sort_records(n, skewed)
    want = take(r, sort_order(r))
    edges = key_edges(want)
    pk = rfx.dyn_pack(r)
    for P in (1, 7, 63):
        s, ps = rfx.dyn_sort_dev(pk, P)
        assert s.n == n
        equals_fast(rfx, s, want, ("sort", n, skewed, P))
        assert ps.cpu().tolist() == partition_starts_np(want, P, edges), ("part_start", n, skewed, P)


# ---- c. the extend pass over more than one scan tile ------------------------------------------------------------------------------------
PASS_FAMILIES = 20_000


def pass_records():
    return M.dyn_crafted_families(np.random.default_rng(83), PASS_FAMILIES, M.DYN_WIDE_LENGTHS)


@pytest.fixture(scope="module")
def pass_set(rfx):
    """about 70,000 crafted rows, sorted (by the numpy order: the model's, see tests/test_scale_inputs.py) -> (model tuples, packed set)"""
    r = host_dyn(pass_records())
    r = take(r, sort_order(r))
    return tuples_of(r, "dyn"), rfx.dyn_pack(r), r


@pytest.mark.parametrize("P", [7, 63])
@pytest.mark.parametrize("stage,start", [(0, 5), (1, 61)])
def test_extend_pass_over_many_tiles(rfx, pass_set, stage, start, P):
    """k_dyn_heads, k_dyn_walk and dyn_emit over ~17 look-back tiles of rows: the records and the output partition starts of
    pymodel.dyn_extend_pass for both start markers"""
    m, pk, r = pass_set
    assert 65_000 < len(m) < 75_000
    s, ps = rfx.dyn_sort_dev(pk, P)
    starts = partition_starts_np(r, P)
    assert ps.cpu().tolist() == starts
    for marker in (1, 2):
        want, want_ops, _ = M.dyn_extend_pass(m, starts, stage, start, marker)
        g, ops = rfx.dyn_extend_pass_dev(s, ps, stage, start, marker)
        equals_fast(rfx, g, host_dyn(want), ("pass", stage, start, P, marker))
        assert ops.cpu().tolist() == want_ops
        assert g.n <= s.n and g.words <= s.words


# ---- d. Count_k_sorted ------------------------------------------------------------------------------------------------------------------
KSORT_GENOME = 20_000


def ksort_rows(k):
    """`KMER,count` rows cut from a random genome, its reverse strand and two variants of it with a changed base every ~300 (one
    read forward, one backward), each k-mer kept with probability 7/8: a sub-k-mer is held by 1 to 4 rows, with one or two extensions"""
    rng = np.random.default_rng(k)
    g = rng.integers(0, 4, KSORT_GENOME + k - 1, dtype=np.uint8)
    rc = lambda s: (3 - s)[::-1]                                   # noqa: E731
    variants = []
    for _ in range(2):
        v = g.copy()
        at = np.arange(150, len(g) - 40, 300)
        at = at + rng.integers(-40, 40, len(at))
        v[at] = (v[at] + rng.integers(1, 4, len(at))) % 4
        variants.append(v)
    rows = []
    for s in (g, rc(g), variants[0], rc(variants[1])):
        text = NUC[s].tobytes().decode()
        keep = rng.random(KSORT_GENOME) < 0.875
        rows += [f"{text[i:i + k]},{int(c)}\n" for i, c in zip(np.flatnonzero(keep), rng.choice(TK.COUNTS, int(keep.sum())))]
    return [rows[i] for i in rng.permutation(len(rows))]


_ksort_cache = {}


def ksort_model_run(k):
    """ksort_rows(k) through ksort_model.run_stages with the default parameters, once per process and k"""
    if k not in _ksort_cache:
        rows, p = ksort_rows(k), K.default_params(k)
        _ksort_cache[k] = dict(rows=rows, p=p, st=K.run_stages(rows, p))
    return _ksort_cache[k]


@pytest.mark.parametrize("k", [31, 95])
def test_ksort_chain_on_70000_rows(rfx, k):
    """~140,000 records: the folds' aggregate scans and the chained sorts past one tile; every stage of the chain composed from the
    operators, the resident chain and its text, against the string model"""
    run = ksort_model_run(k)
    rows, p, want = run["rows"], run["p"], run["st"]
    assert 68_000 < len(rows) < 72_000
    assert {2, 3, 4} <= set(Counter(rec[0] for rec in want["s5_sort"]).values())
    got = TK.chain(rfx, rows, p)
    for s in K.STAGES:
        equals_fast(rfx, got[s], host_kmer(want[s]), (k, s))
    out = rfx.ksort_run(*upload(rows), TK.cparams(rfx, p))
    equals_fast(rfx, out, host_kmer(want["s8"]), (k, "run"))
    assert TK.text_of(rfx, out, k) == K.to_text(want["s8"], k)


# ---- e. Count_k_reduced ------------------------------------------------------------------------------------------------------------------
REDUCE_SEED, REDUCE_GROUPS, REDUCE_K, REDUCE_P = 3, 35_000, (31, 41), 3
REDUCE_SIZES = (65_536, 65_537, 65_793, 131_072, 131_073, None)     # None: the full set
REDUCE_MIN_ROWS = 131_500
_reduce_cache = {}


def reduce_rows():
    """crafted_rows of test_gpu_reduce.py with 35,000 groups -> (short rows, long rows), once per process"""
    if "rows" not in _reduce_cache:
        _reduce_cache["rows"] = crafted_rows(np.random.default_rng(REDUCE_SEED), *REDUCE_K, groups=REDUCE_GROUPS)
    return _reduce_cache["rows"]


def reduce_model_run():
    """reduce_rows() through reduce_model.run_stages, once per process"""
    if "st" not in _reduce_cache:
        st, ps = R.run_stages(*reduce_rows(), *REDUCE_K, REDUCE_P)
        _reduce_cache.update(st=st, ps=ps)
    return _reduce_cache


def pending_trace(recs, right, k1):
    """the two-pending-row loop of reduce_model.adjust over ONE partition, keeping the count only -> (rows pending ahead of each
    row: 0, 1 or 2; the number of rows the loop writes).  Which rows stay pending does not depend on the direction; how many are
    written does"""
    S = lambda x: len(x[0]) == k1 - 1                             # noqa: E731
    P = lambda x, y: R.prefix(x[0], y[0])                         # noqa: E731
    ahead, written = [], 0
    a = b = None
    for c in recs:
        ahead.append(0 if a is None else 1 if b is None else 2)
        if a is None:
            a = c
            continue
        if b is None:
            b = c
            continue
        sa, sb, sc = S(a), S(b), S(c)
        nxt, n_out = "two", 2
        if sa and sb:
            if not sc and P(c, b):
                nxt = "shift"
        elif sa and not sb:
            if sc:
                if P(b, a):
                    n_out = 1 if right else 2
                elif P(c, b):
                    nxt = "shift"
            elif P(b, a) and P(c, a):
                nxt, n_out = "three", 2 if right and (a[1] == b[1] or a[1] == c[1]) else 3
            elif P(b, a):
                n_out = 1 if right else 2
            else:
                nxt = "shift"
        elif not sa and sb:
            if sc:
                if P(a, b):
                    n_out = 1 if right else 2
            elif P(a, b) and P(c, b):
                nxt, n_out = "three", 2 if right and (a[1] == b[1] or b[1] == c[1]) else 3
            elif P(a, b):
                n_out = 1 if right else 2
            elif P(c, b):
                nxt = "shift"
        else:
            if sc and P(a, c) and P(c, b):
                nxt, n_out = "three", 2 if right and (a[1] == c[1] or b[1] == c[1]) else 3
            elif not sc or P(c, b):
                nxt = "shift"
        if nxt == "shift":
            written += 1
            a, b = b, c
        elif nxt == "two":
            written += n_out
            a, b = c, None
        else:
            written += n_out
            a = b = None
    if a is not None and b is not None:
        if S(a) != S(b) and P(a, b):
            written += 1 if right else 2
        elif S(a) or not S(b):
            written += 2
    elif a is not None:
        written += 1
    return ahead, written


def state_variety(ahead):
    """the pending count at the block starts 256 b, b >= 256 (the aggregates a second, third ... one of a thread's stretch in
    k_rd_scan_aggs) -> (how often it is 0, 1, 2; how often it differs from the block start before; the number of block starts)"""
    at = [ahead[i] for i in range(65_536, len(ahead), 256)]
    return [at.count(v) for v in (0, 1, 2)], sum(x != y for x, y in zip(at, at[1:])), len(at)


def reduce_starts(n):
    """P = 5 with cuts on and next to block 256's first row and block 512's, clipped to n and de-duplicated"""
    return sorted({min(x, n) for x in (0, 65_536, 65_537, 100_000, 131_072, n)})


def variety_holds(ahead):
    """every pending count at least twice among the block starts past row 65,536, and a change between consecutive block starts
    for at least a fifth of them"""
    counts, changes, starts = state_variety(ahead)
    return min(counts) >= 2 and 5 * changes >= starts


@pytest.fixture(scope="module")
def reduce_run():
    run = reduce_model_run()
    for right in (False, True):
        recs = run["st"]["right_sort" if right else "left_sort"]
        ahead, _ = pending_trace(recs, right, REDUCE_K[0])
        assert len(recs) >= REDUCE_MIN_ROWS and variety_holds(ahead), (right, len(recs), state_variety(ahead))
    return run


@pytest.mark.parametrize("size", REDUCE_SIZES)
@pytest.mark.parametrize("right", [False, True])
def test_reduce_adjust_where_a_thread_scans_several_block_aggregates(rfx, reduce_run, right, size):
    """k_rd_scan_aggs is one block of 256 threads: from 65,537 rows (257 block aggregates) on a thread composes a stretch of
    ceil(nb / 256) aggregates, threads behind the last stretch have none, and from 131,073 rows on the stretches are of three.
    The first n rows of the sorted set (a prefix of a sorted set is sorted), n on either side of both thresholds, one block past
    the first and the full set; P = 1 and P = 5 with cuts at the thresholds, against the model partition by partition.  The input
    holds every pending count at the block starts past row 65,536, asserted in tests/test_scale_inputs.py."""
    recs = reduce_run["st"]["right_sort" if right else "left_sort"]
    assert len(recs) >= REDUCE_MIN_ROWS
    n = len(recs) if size is None else size
    cp = rfx.reduce_params(*REDUCE_K)
    d = rfx.dyn_pack(host_kmer(recs[:n]))
    for ps in ([0, n], reduce_starts(n)):
        want, _, wps = R.by_partition(lambda r: R.adjust(r, right, REDUCE_K[0]), recs[:n], len(ps) - 1, ps)
        g, gps = rfx.reduce_adjust(d, right, dev_starts(ps), cp)
        equals_fast(rfx, g, host_kmer(want), ("adjust", right, n, ps))
        assert gps.cpu().tolist() == wps and g.n <= d.n


def test_reduce_neutralize_and_the_resident_chain_on_the_full_set(rfx, reduce_run):
    """the same model run: rfx_dev_reduce_neutralize on the sorted full k-mers, and rfx_dev_reduce_run from the two texts -- the set
    and both final texts"""
    st, ps = reduce_run["st"], reduce_run["ps"]
    rs, rl = reduce_run["rows"]
    cp = rfx.reduce_params(*REDUCE_K)
    g, gps = rfx.reduce_neutralize(rfx.dyn_pack(host_kmer(st["full_sort"])), dev_starts(ps["full_sort"]), cp)
    want = host_kmer(st["neutral"])
    equals_fast(rfx, g, want, "neutralize")
    assert gps.cpu().tolist() == ps["neutral"]
    out = rfx.reduce_run(*upload(lines(rs)), *upload(lines(rl)), REDUCE_P, cp)
    equals_fast(rfx, out, want, "run")
    for k in REDUCE_K:
        assert TK.text_of(rfx, out, k) == R.to_text(st["neutral"], k), ("text", k)


# ---- f. 04Fixing --------------------------------------------------------------------------------------------------------------------------
def test_fixing_chain_on_5000_contigs(rfx, monkeypatch):
    """more contigs than one scan tile (rfx_find's offset arrays, k_fx_ends_kmers / k_fx_ends_long), ~24,000 union rows, six tiles in
    both folds: chain_equals_model of test_gpu_fixing.py as it is, its raw-word comparison on the vectorised packer"""
    monkeypatch.setattr(TF, "raw_equals", raw_equals_fast)
    rows = TF.contig_rows(np.random.default_rng(5000), 5000, 32)
    want, passes = TF.chain_equals_model(rfx, rows, F.default_params(32, max_iteration=1), 7, "5000 contigs")
    assert len(want["binarized"]) == 5000 and len(want["union"]) > 20_000 and len(passes[-1]) < len(want["fold2"])


KMER_SET_N, KMER_SET_DUPS, KMER_SET_LONGS = 420_000, 60_000, 50


def kmer_set_input():
    """420,000 31-mer values below 2^62 in random order, 60,000 of them repeats of earlier ones, and 50 long records"""
    rng = np.random.default_rng(62)
    v = np.unique(rng.integers(0, 1 << 62, KMER_SET_N - KMER_SET_DUPS + 64, dtype=np.int64))[:KMER_SET_N - KMER_SET_DUPS]
    v = rng.permutation(np.concatenate([v, rng.choice(v, KMER_SET_DUPS)]))
    longs = [(TF.rand_seq(rng, 30), 1, TF.rand_seq(rng, 2 + 7 * j), int(rng.choice(TF.MARK)), int(rng.choice(TF.MARK))) for j in range(KMER_SET_LONGS)]
    return v, longs


def kmer_set_records(v, longs):
    """np.unique: the distinct values ascending, key = the first 30 bases, extension = the last, attributes (1, -1, -1); the long
    records behind them"""
    u = np.unique(v).astype(np.uint64)
    n = len(u)
    codes = ((u[:, None] >> (np.uint64(60) - np.uint64(2) * np.arange(31, dtype=np.uint64))) & np.uint64(3)).astype(np.uint8)
    minus = np.full(n, -1)
    kmers = dyn_records(codes[:, :30].reshape(-1), np.arange(n + 1) * 30, codes[:, 30], np.arange(n + 1), np.ones(n), minus, minus)
    return concat(kmers, host_dyn(longs)), n


def test_fixing_kmer_set_sorts_62_bits_on_the_two_level_path(rfx):
    """420,000 values are more than 192 sort tiles: sort_pairs takes two MSD levels on 62-bit keys inside the stage"""
    import torch
    v, longs = kmer_set_input()
    want, distinct = kmer_set_records(v, longs)
    assert len(v) == KMER_SET_N and distinct == KMER_SET_N - KMER_SET_DUPS
    d_v = torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    u = rfx.fix_kmer_set(d_v, len(v), rfx.dyn_pack(host_dyn(longs)))
    assert u.n == distinct + KMER_SET_LONGS
    equals_fast(rfx, u, want, "kmer set")
    key = u.host()[0]
    assert np.array_equal(key[:distinct, 0] >> np.uint64(4), np.unique(v).astype(np.uint64) >> np.uint64(2))


FORK_N, FORK_RUNS, FORK_EDGES = 270_000, 3000, (4096, 8192, 262_144)
FORK_KINDS = ("ones", "ones then longs", "mixed", "ties")
_fork_cache = {}


def fork_run(kind, key, m, ln, rng):
    one = lambda ch, j: (key, m, ch, -1 - j, j)                    # noqa: E731
    lng = lambda j: (key, m, TF.rand_seq(rng, 2 + 31 * (j % 4)), j, -j)        # noqa: E731
    if kind == "ones":
        return [one("GCTGTCGG"[j % 8], j) for j in range(ln)]
    if kind == "ones then longs":
        cut = max(1, ln * 14 // 24)
        return [one("ACGT"[j % 4], j) for j in range(cut)] + [lng(j) for j in range(cut, ln)]
    if kind == "mixed":
        return [lng(j) if j % 12 in (3, 11) or j == ln - 1 else one("ACGT"[j % 4], j) for j in range(ln)]
    return [one("TCGC"[j % 4], j) for j in range(ln)]


def fork_records(reflected):
    """270,000 sorted rows with 30-base keys, built the way test_a_run_of_equal_keys_across_a_block_edge builds its 600: a key holds
    one row (one-base, or longer for every third key) or is one of 3,000 runs of 2 to 40 rows, the four kinds in turn; runs of 24
    rows lie across rows 4,096, 8,192 and 262,144 (12 rows on either side) -> (records, [(first row, length, kind)])"""
    if reflected in _fork_cache:
        return _fork_cache[reflected]
    rng = np.random.default_rng(270 + int(reflected))
    m = 2 if reflected else 1
    lens = np.ones(FORK_N, np.int64)                               # rows per key, more keys than needed
    lens[rng.choice(200_000, FORK_RUNS + 10, replace=False)] = rng.integers(2, 41, FORK_RUNS + 10)
    for edge in FORK_EDGES:                                        # a key whose first row is edge - 12 becomes a run of 24
        first = offsets_of(lens)
        k = int(np.searchsorted(first, edge - 12, side="right")) - 1
        if first[k] < edge - 12:                                   # (cut the key there short so that the next one starts on edge - 12)
            lens[k] = edge - 12 - first[k]
            k += 1
        lens[k] = 24
    first = offsets_of(lens)
    nk = int(np.searchsorted(first, FORK_N, side="left"))          # keys 0 .. nk - 1 cover FORK_N rows, the last one cut short
    lens = lens[:nk].copy()
    lens[-1] -= first[nk] - FORK_N
    vals = np.unique(rng.integers(0, 1 << 60, nk + 64, dtype=np.int64))[:nk].astype(np.uint64)
    vals = vals[np.argsort((vals ^ (np.uint64(1) << np.uint64(59))), kind="stable")]                   # signed first block: G < T < A < C
    codes = ((vals[:, None] >> (np.uint64(58) - np.uint64(2) * np.arange(30, dtype=np.uint64))) & np.uint64(3)).astype(np.uint8)
    keys = strings_of(codes.reshape(-1), np.arange(nk + 1) * 30)
    recs, runs, kind_at = [], [], 0
    for i, (key, ln) in enumerate(zip(keys, lens.tolist())):
        if ln == 1:
            recs.append((key, m, "ACGT"[int(rng.integers(0, 4))], -1 - i % 20000, i % 20000) if i % 3 else (key, m, TF.rand_seq(rng, 2 + 31 * (i % 4)), i % 20000, -(i % 20000)))
        else:
            kind = FORK_KINDS[kind_at % 4]
            kind_at += 1
            runs.append((len(recs), ln, kind))
            recs += fork_run(kind, key, m, ln, rng)
    _fork_cache[reflected] = (recs, runs)
    return recs, runs


@pytest.mark.parametrize("P", [1, 63])
@pytest.mark.parametrize("reflected", [False, True])
def test_fixing_fork_filter_on_270000_rows(rfx, reflected, P):
    """the fold's flag scans over 66 look-back tiles, runs of equal keys across tile edges and across the first row a second lane
    window serves: against the closed form of the fold partition by partition (the fold itself on a 20,000-row slice)"""
    recs, runs = fork_records(reflected)
    n = len(recs)
    assert n == FORK_N
    r = host_dyn(recs)
    ps = partition_starts_np(r, P)
    want, _, wps = F.by_partition(F.fold_closed_form, recs, P, ps)
    cut = slice(250_000, 270_000)
    assert F.fold(recs[cut]) == F.fold_closed_form(recs[cut])
    g, gps = rfx.fix_fork_filter(rfx.dyn_pack(r), reflected, dev_starts(ps))
    equals_fast(rfx, g, host_dyn(want), ("fork filter", reflected, P))
    assert gps.cpu().tolist() == wps


# ---- g. poisoned allocations ---------------------------------------------------------------------------------------------------------------
def test_the_reduce_and_fixing_tests_hold_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it; the tests of the
    reduction and the fixing stage above, in a child process (the mask is read once per process)"""
    import subprocess
    import sys
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "(reduce or fixing) and not poisoned"],
                       env=env, cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
