"""The dynamic-k entries (rfx_dyn_sort, rfx_dyn_random_reflection, rfx_dyn_extend_pass, rfx_dyn_run) where tests/test_gpu_dynamic.py
does not reach: keys at the 31-base block edges and up to 124 bases, the order of the block form, every rule of the pass with keys
of different lengths (counted by the string model's census), the walk's 128-row blocks and the 256-thread kernels, P up to 63 with
empty partitions, and the refusals.  Three statements are compared FIELD BY FIELD: the kernels, the oracle
(oracle/reflexiv_dynamic.c) and the string model (tests/pymodel.py); tests/test_oracle_dynamic.py holds the latter two against
rows made by the reference's own classes (tests/golden/dynamic_edge_vectors.npz), which the first test here feeds to the kernels."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import pymodel as M
from tests.test_oracle_dynamic import EDGE, edge_cases, rows_of, model_rows

pytestmark = pytest.mark.gpu

OK, E_ARG, E_LIMIT = 0, -1, -6
FILL = 0xA5
NUC = "ACGT"


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


def dev(recs):
    from reflexiv_amd.api import DynRecords
    return DynRecords.from_rows(model_rows(recs))


def orc(recs):
    return O.dyn_binarize_rows(model_rows(recs))


def same_records(g, o, tag):
    """two record sets field by field: offsets, bases, marker, left, right"""
    assert g.n == o.n, (tag, "n", g.n, o.n)
    for f in ("key_off", "ext_off", "marker", "left", "right"):
        a, b = np.asarray(getattr(g, f))[:g.n + (f.endswith("off"))], np.asarray(getattr(o, f))[:o.n + (f.endswith("off"))]
        if not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0]) if a.shape == b.shape else -1
            raise AssertionError((tag, f, i, a[i] if i >= 0 else a.shape, b[i] if i >= 0 else b.shape))
    for f, off in (("key", "key_off"), ("ext", "ext_off")):
        a, b = getattr(g, f)[:int(getattr(g, off)[g.n])], getattr(o, f)[:int(getattr(o, off)[o.n])]
        assert np.array_equal(a, b), (tag, f, int(np.flatnonzero(a != b)[0]))


def same_rows(g, want, tag):
    rows = g.rows()
    assert len(rows) == len(want), (tag, len(rows), len(want))
    for i, (a, b) in enumerate(zip(rows, want)):
        assert a == b, (tag, i, a, b)


def sorted_three_ways(rfx, recs, Ps, tag):
    """rfx_dyn_sort against the oracle's order and the model's, and the cut for every P -> the sorted set (device form, oracle
    form, model form)"""
    o = O.dyn_sort(orc(recs))
    m = M.dyn_sort(recs)
    assert o.rows() == model_rows(m), (tag, "oracle against model")
    g = None
    for P in Ps:
        g, ps = rfx.dyn_sort(dev(recs), P)
        same_records(g, o, (tag, "sort", P))
        want = O.dyn_partition_starts(o, P)
        assert np.array_equal(ps, want), (tag, "part_start", P, ps, want)
        assert list(want) == M.dyn_partition_starts(m, P), (tag, "oracle's cut against the model's", P)
    return g, o, m


def pass_three_ways(rfx, g, o, m, P, stage, start, start_marker, tag):
    """rfx_dyn_extend_pass against the oracle and the model on one sorted set -> (device output, the model's labels)"""
    ps = O.dyn_partition_starts(o, P)
    want, want_ops = O.dyn_extend_pass(o, ps, stage, start, start_marker)
    got, ops = rfx.dyn_extend_pass(g, ps, stage, start, start_marker)
    same_records(got, want, tag)
    assert np.array_equal(ops, want_ops), (tag, "out_part_start", ops, want_ops)
    out, mops, labels = M.dyn_extend_pass(m, [int(x) for x in ps], stage, start, start_marker)
    same_rows(got, model_rows(out), (tag, "model"))
    assert [int(x) for x in ops] == mops, (tag, "out_part_start against the model", ops, mops)
    return got, labels


# ---- the reference-made edge vectors -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", edge_cases())
def test_gpu_operators_equal_the_reference_classes_on_crafted_families(rfx, case):
    """sort, partition starts, each pass and out_part_start on the rows the reference's own classes gave for crafted families
    (keys of 22..94 bases at the block edges, every distance branch, the rules from iteration 61 on, the clamp, start marker 1),
    every pass fed with the reference's previous output"""
    from reflexiv_amd.api import DynRecords
    z = np.load(EDGE)
    P, stage, start, start_marker, passes = (int(x) for x in z[case + "/meta"])
    prev = rows_of(z, case + "/in")
    for i in range(passes):
        o = O.dyn_sort(O.dyn_binarize_rows(prev))
        g, ps = rfx.dyn_sort(DynRecords.from_rows(prev), P)
        same_records(g, o, (case, i, "sort"))
        assert np.array_equal(ps, O.dyn_partition_starts(o, P)), (case, i, "part_start")
        got, ops = rfx.dyn_extend_pass(g, ps, stage, start, start_marker)
        want = rows_of(z, f"{case}/pass{i}")
        same_rows(got, want, (case, i, "pass"))
        _, want_ops = O.dyn_extend_pass(o, ps, stage, start, start_marker)
        assert np.array_equal(ops, want_ops), (case, i, "out_part_start", ops, want_ops)
        prev = want


# ---- the order of the block form ---------------------------------------------------------------------------------------------
SORT_LENGTHS = (1, 2, 30, 31, 32, 33, 61, 62, 63, 64, 92, 93, 94, 95, 123, 124)
G_BLOCK = "G" + 30 * "A"                                   # 0x8000...0 as a non-last block: the sort key's sign flip makes it 0


def sort_keys():
    """hand-built keys for the order of array<long> (signed blocks, a proper prefix first)"""
    rng = np.random.default_rng(31)
    rnd = lambda n: "".join(NUC[b] for b in rng.integers(0, 4, n))
    keys = []
    base = rnd(124)
    for L in SORT_LENGTHS:                                  # every length, every block starting with every base
        for b in NUC:
            k = list(base[:L])
            for j in range(0, L, 31):
                k[j] = b
            keys.append("".join(k))
        keys += [base[:L - 1] + b for b in NUC]             # ... and keys that differ only in the last base of the last block
    for j in range(3):                                      # G + 30 x A as block j, not the last block
        head = base[:31 * j]
        for tail in ("A", "C", "T" + rnd(7), G_BLOCK, rnd(31) + "C")[:5 if j < 2 else 4]:
            if len(head + G_BLOCK + tail) <= 124:
                keys.append(head + G_BLOCK + tail)
        keys.append(head + G_BLOCK)                         # (as the LAST block: 0x8000...1)
        keys.append(head + "A" * 31 + "C")                  # (a block of zeros beside it)
        if j:
            keys += [head, head[:-1], head[:-1] + "C"]      # keys that end before that block
        # a key whose terminator reads as the longer key's C + A...A: blocks equal up to its last, then a proper prefix --
        # next to longer keys whose next block is G + 30 x A (0 after the flip, like an absent block) and A...A
        for t in (0, 5, 30):
            short = head + base[31 * j:31 * j + t]
            full = short + "C" + "A" * (30 - t)
            keys += [short, full + G_BLOCK + "T", full + "A" * 31, full + "T"]
    for cut in (31, 62, 93):                                # base-prefixes at a block's end next to their one-base-longer keys
        keys.append(base[:cut])
        keys += [base[:cut] + b for b in NUC]
        keys.append(base[:cut - 1])
    keys = [k for k in keys if 1 <= len(k) <= 124]
    keys += keys[::7] + keys[::7] + keys[::11]              # duplicates: stability shows in the attributes
    return keys


def sort_records():
    rng = np.random.default_rng(32)
    keys = sort_keys()
    keys = [keys[i] for i in rng.permutation(len(keys))]
    # (left = the input position: unique, so the order of equal keys is visible)
    return [(k, 1 + i % 2, "".join(NUC[b] for b in rng.integers(0, 4, 1 + i % 5)), i, -1 - i) for i, k in enumerate(keys)]


def test_sort_order_of_the_block_form(rfx):
    """keys of every length around the block edges, each block starting with each base, G + 30 x A as a non-last block (the
    sign flip makes it 0, the value of an absent block), base-prefixes of 31 / 62 / 93 bases next to their longer keys, duplicates:
    the order and the cut against the oracle and the model, field by field"""
    recs = sort_records()
    assert 250 <= len(recs) <= 1000 and max(len(r[0]) for r in recs) == 124 and {len(r[0]) for r in recs} >= set(SORT_LENGTHS)
    g, o, m = sorted_three_ways(rfx, recs, (1, 2, 5, 63), "hand-built keys")
    order = [r[0] for r in m]
    # what the header says about this order, on the model: a 31-base key sorts AFTER the 32-base key it is a base-prefix of (its
    # block carries the terminator in bit 0); blocks that start with G or T are negative and sort first; equal keys keep their order
    base31 = next(k for k in order if len(k) == 31 and any(x[:31] == k and len(x) == 32 for x in order))
    assert order.index(base31) > max(i for i, x in enumerate(order) if len(x) == 32 and x[:31] == base31)
    assert order[0][0] in "GT" and order[-1][0] in "AC"
    for a, b in zip(m, m[1:]):
        assert a[0] != b[0] or a[3] < b[3]


class DynScratch:
    """output records, part_start, out_part_start and trace filled with 0xA5, sentinels in the struct's scalars and *n_trace"""
    SENT = -77

    def __init__(self):
        from reflexiv_amd.api import DynRecords
        self.out = DynRecords.empty(64, 8192, 8192)
        self.ps, self.ops, self.trace = np.empty(65, np.int64), np.empty(65, np.int64), np.empty(16, np.int64)
        self.arrays = [self.out.key, self.out.key_off, self.out.ext, self.out.ext_off, self.out.marker, self.out.left, self.out.right,
                       self.ps, self.ops, self.trace]
        for a in self.arrays:
            a.view(np.uint8).fill(FILL)
        self.co = self.out._c()
        self.co.n = self.co.need_key = self.co.need_ext = self.SENT
        self.co.cap_n, self.co.cap_key, self.co.cap_ext = 64, 8192, 8192
        self.ntr = C.c_int64(self.SENT)

    def untouched(self):
        return (all(bool((a.view(np.uint8) == FILL).all()) for a in self.arrays) and self.ntr.value == self.SENT
                and (self.co.n, self.co.need_key, self.co.need_ext) == (self.SENT,) * 3)


def dyn_entries(rfx, r, P, s):
    """the four entries on the scratch outputs -> {name: thunk that returns the status}"""
    from reflexiv_amd.api import _p
    L, ctx = rfx.L, rfx.ctx
    ci = r._c()
    part = np.zeros(65, np.int64)
    part[1:] = r.n                                           # one partition with every row, the others empty
    s.keep = r                                               # (ci holds bare pointers into r's arrays)
    return {
        "rfx_dyn_sort": lambda: L.rfx_dyn_sort(ctx, C.byref(ci), P, C.byref(s.co), _p(s.ps)),
        "rfx_dyn_random_reflection": lambda: L.rfx_dyn_random_reflection(ctx, C.byref(ci), _p(part), P, C.byref(s.co)),
        "rfx_dyn_extend_pass": lambda: L.rfx_dyn_extend_pass(ctx, C.byref(ci), _p(part), P, 1, 5, 2, C.byref(s.co), _p(s.ops)),
        "rfx_dyn_run": lambda: L.rfx_dyn_run(ctx, C.byref(ci), P, 1, 1, 5, 5, C.byref(s.co), _p(s.trace), C.c_int64(16), C.byref(s.ntr)),
    }


def test_a_key_of_125_bases_is_refused(rfx):
    """124 bases are four blocks and pass; one key of 125 among them gives RFX_E_LIMIT from all four entries (the sorting ones
    find it on the device, the other two on the host), with every output buffer and scalar as it was"""
    rng = np.random.default_rng(33)
    recs = [("".join(NUC[b] for b in rng.integers(0, 4, L)), 1 + i % 2, "ACG"[:1 + i % 3], -3, -4) for i, L in enumerate((40, 124, 94, 124, 31))]
    for name in ("rfx_dyn_sort", "rfx_dyn_random_reflection", "rfx_dyn_extend_pass", "rfx_dyn_run"):
        s = DynScratch()
        assert dyn_entries(rfx, dev(recs), 2, s)[name]() == OK, name
        assert not s.untouched()
    long = recs[:3] + [("".join(NUC[b] for b in rng.integers(0, 4, 125)), 1, "A", -3, -4)] + recs[3:]
    for name in ("rfx_dyn_sort", "rfx_dyn_random_reflection", "rfx_dyn_extend_pass", "rfx_dyn_run"):
        s = DynScratch()
        assert dyn_entries(rfx, dev(long), 2, s)[name]() == E_LIMIT, name
        assert s.untouched(), name


@pytest.mark.parametrize("P", [0, 64, -1])
def test_a_partition_count_out_of_range_is_refused(rfx, P):
    """P = 0 and P = 64 (the entries take 1..63): RFX_E_ARG from all four, outputs untouched"""
    recs = M.dyn_crafted_families(np.random.default_rng(34), 3)
    for name in ("rfx_dyn_sort", "rfx_dyn_random_reflection", "rfx_dyn_extend_pass", "rfx_dyn_run"):
        s = DynScratch()
        assert dyn_entries(rfx, dev(recs), P, s)[name]() == E_ARG, name
        assert s.untouched(), name


# ---- the rules of the pass ----------------------------------------------------------------------------------------------------
PASS_CONFIGS = [(0, 0, 15), (1, 5, 40), (1, 61, 40)]        # stage, start iteration, longest extension (stage 0: see DESIGN.md)
_crafted = {}


def crafted(stage, start, ext_max):
    if (stage, start) not in _crafted:
        _crafted[stage, start] = M.dyn_crafted_families(np.random.default_rng(100 + stage + start), 900, M.DYN_WIDE_LENGTHS, ext_max)
    return _crafted[stage, start]


@pytest.mark.parametrize("start_marker", [2, 1])
@pytest.mark.parametrize("stage,start,ext_max", PASS_CONFIGS)
def test_pass_rules_on_crafted_families(rfx, stage, start, ext_max, start_marker):
    """900 crafted families (about 3000 records, keys of 22..124 bases, P = 7) through one pass, against the oracle and the model
    field by field with out_part_start.  The model's census keeps the set honest: every decision the configuration can reach is
    taken at least 3 times, and so is each of the two where `- extra` alone decides a distance branch."""
    recs = crafted(stage, start, ext_max)
    assert len(recs) < 4000 and {len(r[0]) for r in recs} == set(M.DYN_WIDE_LENGTHS)
    g, o, m = sorted_three_ways(rfx, recs, (7,), (stage, start))
    _, labels = pass_three_ways(rfx, g, o, m, 7, stage, start, start_marker, (stage, start, start_marker))
    census = M.dyn_census(labels)
    print("census", stage, start, start_marker, sorted(census.items(), key=lambda t: t[1]))
    assert set(census) <= set(M.dyn_labels(stage, start) + M.DYN_LABELS_EXTRA_DECIDES), sorted(census)
    short = {lb: census.get(lb, 0) for lb in M.dyn_labels(stage, start) + M.DYN_LABELS_EXTRA_DECIDES if census.get(lb, 0) < 3}
    assert not short, short


# ---- the decomposition: families, heads, bases, parity, offsets -----------------------------------------------------------------
DECOMP_P = (1, 2, 5, 31, 63)


def decomposition(rfx, recs, tag, Ps=DECOMP_P, configs=((0, 0, 2), (1, 5, 1), (1, 61, 2))):
    """sort + cut for every P, then a pass per P (the configurations in turn) and the random reflection on the cut"""
    g, o, m = sorted_three_ways(rfx, recs, Ps, tag)
    if g is None:
        return
    for i, P in enumerate(Ps):
        stage, start, start_marker = configs[i % len(configs)]
        pass_three_ways(rfx, g, o, m, P, stage, start, start_marker, (tag, P, stage, start, start_marker))
        ps = O.dyn_partition_starts(o, P)
        same_records(rfx.dyn_random_reflection(g, ps), O.dyn_random_reflection(o, ps), (tag, P, "random reflection"))


@pytest.mark.parametrize("n", [0, 1, 2, 127, 128, 129, 255, 256, 257, 2049])
def test_decomposition_at_the_block_edges(rfx, n):
    """n around the walk's 128-row blocks and the 256-thread kernels, 2049 beyond one sort tile; P up to 63, also P > n"""
    recs = M.dyn_crafted_families(np.random.default_rng(200 + n), n // 3 + 2, M.DYN_WIDE_LENGTHS)
    while len(recs) < n:
        recs += M.dyn_crafted_families(np.random.default_rng(len(recs)), 8, M.DYN_WIDE_LENGTHS)
    decomposition(rfx, recs[:n], ("n", n))


def test_decomposition_with_one_base_keys(rfx):
    """the shortest key has 1 base, so a family is every key that starts with the same base: several hundred rows walked by one
    thread, across many 128-row blocks, and partitions that start inside a family"""
    rng = np.random.default_rng(41)
    recs = M.dyn_crafted_families(rng, 330, M.DYN_WIDE_LENGTHS)
    recs += [(b, 1 + i % 2, "ACGT"[:1 + i], (-5, 0, 12, 50)[i], (7, -2, 0, -9)[i]) for i, b in enumerate(NUC)] + [("A", 2, "TT", 3, -1)]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    assert min(len(r[0]) for r in recs) == 1 and len(recs) > 900
    decomposition(rfx, recs, "one-base keys")


def equal_run(rng, key, count):
    return [(key, int(rng.integers(1, 3)), "".join(NUC[b] for b in rng.integers(0, 4, int(rng.integers(1, 20)))),
             M.dyn_crafted_attribute(rng), M.dyn_crafted_attribute(rng)) for _ in range(count)]


def test_decomposition_with_a_long_run_of_equal_keys(rfx):
    """a run of more than n / P equal keys: several cuts collapse onto the end of the run and leave empty partitions"""
    rng = np.random.default_rng(42)
    recs = M.dyn_crafted_families(rng, 100, M.DYN_WIDE_LENGTHS)
    key = recs[len(recs) // 2][0]
    recs += equal_run(rng, key, 400)
    recs = [recs[i] for i in rng.permutation(len(recs))]
    m = M.dyn_sort(recs)
    for P in (5, 31, 63):
        st = M.dyn_partition_starts(m, P)
        assert sum(a == b for a, b in zip(st, st[1:])) >= 2, (P, st)            # empty partitions behind the collapsed cuts
    decomposition(rfx, recs, "a long run")


def test_decomposition_with_a_run_of_equal_keys_that_ends_at_n(rfx):
    """the last key of the order repeated 300 times: the cuts inside the run move to n, and the last partitions are empty"""
    rng = np.random.default_rng(43)
    recs = M.dyn_crafted_families(rng, 60, M.DYN_WIDE_LENGTHS)
    key = "C" + "T" * 93                                      # (blocks that start with C are the largest signed values)
    recs += equal_run(rng, key, 300)
    recs = [recs[i] for i in rng.permutation(len(recs))]
    m = M.dyn_sort(recs)
    assert [r[0] for r in m[-300:]] == [key] * 300
    st = M.dyn_partition_starts(m, 5)
    assert st[-2] == len(recs) and st[-1] == len(recs), st
    decomposition(rfx, recs, "a run that ends at n")


def test_a_partition_whose_rows_are_all_dropped_but_one(rfx):
    """From iteration 61 on a forward row shorter than the reflected holder is dropped.  A non-empty partition can never emit
    NOTHING -- its first row becomes the holder, and a holder leaves only by being emitted, merged or dropped beside an emitted
    row -- so the smallest output is one row.  Five families of 31 rows: one reflected 124-base key, then thirty shorter forward
    base-prefixes of it (the family has A behind every prefix, so each sorts after the full key).  At P = 5 every partition is one
    family and emits exactly its holder; at P = 31 and 63 partitions start inside a family, others are empty, and out_part_start,
    the bases and the parity of every later partition depend on these counts."""
    rng = np.random.default_rng(44)
    lengths = (22, 30, 31, 40, 61, 62, 80, 93, 95, 110)
    recs = []
    for f in range(5):
        fam = list(NUC[b] for b in rng.integers(0, 4, 124))
        for L in lengths:
            fam[L] = "A"
        fam = "".join(fam)
        recs.append((fam, 2, "ACG", -4, -6))
        recs += [(fam[:L], 1, "TG"[:1 + i % 2], -2 - i, -3) for i in range(3) for L in lengths]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    m = M.dyn_sort(recs)
    for P in (1, 5, 31, 63):
        st = M.dyn_partition_starts(m, P)
        out, ost, labels = M.dyn_extend_pass(m, st, 1, 61)
        counts = [(b - a, d - c) for a, b, c, d in zip(st, st[1:], ost, ost[1:])]
        assert all(e >= 1 for rows, e in counts if rows) and all(e == 0 for rows, e in counts if not rows), counts
        if P == 1:
            assert len(out) == 5 and M.dyn_census(labels)["forward row shorter: dropped"] == 150
        if P == 5:
            assert counts == [(31, 1)] * 5, counts
    decomposition(rfx, recs, "dropped rows", Ps=(1, 5, 31, 63), configs=((1, 61, 2), (1, 61, 1)))


def test_random_reflection_on_given_partitions_at_63(rfx):
    """rfx_dyn_random_reflection on a hand-given part_start: 63 partitions, many of them empty (at the front, in the middle, at
    the end), odd and even sizes, so the orientation of a row depends on finding its own partition among equal starts"""
    recs = M.dyn_crafted_families(np.random.default_rng(45), 120, M.DYN_WIDE_LENGTHS)
    n = len(recs)
    cuts = sorted([0, 0, 0, 1, 1, 4, 9, 9, 9, 9, 130, 131, n - 3, n - 3, n] + [int(x) for x in np.random.default_rng(46).integers(0, n, 35)])
    st = np.array(cuts + [n] * (64 - len(cuts)), np.int64)
    assert len(st) == 64 and st[0] == 0 and st[-1] == n
    got = rfx.dyn_random_reflection(dev(recs), st)
    same_records(got, O.dyn_random_reflection(orc(recs), st), "random reflection at P = 63")
    same_rows(got, model_rows(M.dyn_random_reflection(recs, [int(x) for x in st])), "random reflection against the model")


# ---- the drivers ---------------------------------------------------------------------------------------------------------------
def test_drivers_at_63_partitions(rfx):
    """rfx_dyn_run on crafted families at P = 63: the first four passes (after the random reflection), then iterations 61..63
    under the rules from 61 on, against the oracle's drivers and the model's chain, with the trace"""
    recs = M.dyn_crafted_families(np.random.default_rng(47), 500, M.DYN_WIDE_LENGTHS, ext_max=1)
    kmers = [(k + e, f"1|{l}|{r}") for k, _, e, l, r in recs]                   # FirstFour's input: (k-mer, attribute) rows
    P = 63
    from reflexiv_amd.api import DynRecords
    want_ff, tr_ff = O.dyn_first_four(kmers, P)
    ff, tr = rfx.dyn_run(DynRecords.from_kmer_rows(kmers), P, random_reflection=True, passes_first_four=4)
    same_records(ff, O.dyn_binarize_rows(want_ff), "first four")
    assert tr == [len(rows) for tag, rows in tr_ff if tag.startswith("extend")]
    want, tr_it = O.dyn_iterations(want_ff, P, 61, 63)
    fin, tr = rfx.dyn_run(DynRecords.from_rows(want_ff), P, start_iteration=61, end_iteration=63)
    same_records(fin, O.dyn_binarize_rows(want), "iterations 61..63")
    assert tr == [len(rows) for tag, rows in tr_it if tag.startswith("it_extend")] and len(tr) == 3
    # the model's chain
    m = [(k[:-1], 1, k[-1], int(a.split("|")[1]), int(a.split("|")[2])) for k, a in kmers]
    m = M.dyn_random_reflection(m, [p * len(m) // P for p in range(P)] + [len(m)])
    for stage, start in [(0, 0)] * 4 + [(1, 61)] * 3:
        m = M.dyn_sort(m)
        m, _, _ = M.dyn_extend_pass(m, M.dyn_partition_starts(m, P), stage, start)
        if (stage, start) == (0, 0):
            ff_model = m
    assert model_rows(ff_model) == want_ff
    same_rows(fin, model_rows(m), "iterations against the model")
