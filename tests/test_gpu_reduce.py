"""The k-mer reduction stage (Count_<k1>_reduced, Count_<k2>_sorted / _reduced) on packed record sets in HBM (rfx_dev_reduce_*,
rfx_reduce_text): every operator against its stage of the rows the reference's own classes made
(tests/golden/reduce_vectors.npz), unpacked field by field and as raw words against the numpy packer; the resident chain and the
host form against both final texts; row counts around the block size, a long run of long rows that keeps two rows pending across
block edges, partitions of 0..3 rows and partition starts on and past a block edge, the neutralizer's drop stretch across a block
edge -- against the string model (tests/reduce_model.py, which test_reduce_model.py pins to the same vectors); the argument, capacity
and text-buffer contracts; the hand-over from the sorting stage and to rfx_dev_dyn_binarize form 0; and all of it again with every
allocation poisoned."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import reduce_model as R
from tests.test_gpu_dynamic_edges import same_records
from tests.test_gpu_dynamic_packed import raw_equals, poisoned, untouched, FILL, OK, E_ARG, E_CAP
from tests.test_gpu_ksort import host, upload, text_of

pytestmark = pytest.mark.gpu

VEC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduce_vectors.npz")
MARK = (-1, -3, 1, 2, 7, 100, 30000)


def case_names(twins=True):
    return [str(x) for x in np.load(VEC)["names"] if twins or "_m" not in str(x)]


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


@pytest.fixture(scope="module")
def vec():
    """every case, loaded once: name -> (meta, short rows, long rows, {stage: records}, {stage: part starts}, text 1, text 2)"""
    z = np.load(VEC)
    return {n: R.load_case(z, n) for n in case_names()}


def cparams(rfx, meta):
    return rfx.reduce_params(meta["k1"], meta["k2"], max_k=meta["max_k"])


def lines(rows):
    return [r if r.endswith("\n") else r + "\n" for r in rows]


def dev_starts(ps):
    import torch
    t = torch.tensor([int(x) for x in ps], dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    return t


def equals(rfx, pk, recs, tag):
    """the packed set in HBM is the record list: unpacked field by field, and word for word the numpy packer's"""
    want = host(recs)
    same_records(rfx.dyn_unpack(pk), want, tag)
    raw_equals(pk, want, tag)


def rand_seq(rng, n):
    return "".join("ACGT"[b] for b in rng.integers(0, 4, n))


def crafted_rows(rng, k1, k2, groups=24):
    """two small inputs in which short rows meet longer rows on their left and on their right, with equal and unequal extensions
    and markers of either sign"""
    attr = lambda: f"1|{int(rng.choice(MARK))}|{int(rng.choice(MARK))}"                       # noqa: E731
    g = rand_seq(rng, 40 + k2)
    rs = [f"{g[i:i + k1]},{attr()}" for i in range(0, 30)]
    rl = [f"{g[i:i + k2]},{attr()}" for i in range(10, len(g) - k2 + 1)]
    d = k2 - k1
    for j in range(groups):
        core = rand_seq(rng, k1)
        if j % 4 != 3:
            rs.append(f"{core},{attr()}")
        for _ in range(int(rng.integers(0, 4))):
            e = core[-1] if rng.random() < 0.5 else "ACGT"[int(rng.integers(0, 4))]
            rl.append(f"{rand_seq(rng, d)}{core[:-1]}{e},{attr()}")
        for _ in range(int(rng.integers(0, 4))):
            f = core[0] if rng.random() < 0.5 else "ACGT"[int(rng.integers(0, 4))]
            rl.append(f"{f}{core[1:]}{rand_seq(rng, d)},{attr()}")
    return rs, rl


def chain(rfx, rows_s, rows_l, meta):
    """the operators one by one on the device, each on the device's previous output -> {stage: packed set}, {stage: part starts}"""
    cp, P = cparams(rfx, meta), meta["P"]
    st, ps = {}, {}
    st["union"] = rfx.reduce_union(*upload(lines(rows_s)), *upload(lines(rows_l)), cp)
    st["left_prep"] = rfx.reduce_left_prepare(st["union"], cp)
    st["left_sort"], ps["left_sort"] = rfx.dyn_sort_dev(st["left_prep"], P)
    st["left_adj"], ps["left_adj"] = rfx.reduce_adjust(st["left_sort"], False, ps["left_sort"], cp)
    st["right_prep"] = rfx.reduce_right_prepare(st["left_adj"], cp)
    st["right_sort"], ps["right_sort"] = rfx.dyn_sort_dev(st["right_prep"], P)
    st["right_adj"], ps["right_adj"] = rfx.reduce_adjust(st["right_sort"], True, ps["right_sort"], cp)
    st["full"] = rfx.reduce_full_kmers(st["right_adj"], cp)
    st["full_sort"], ps["full_sort"] = rfx.dyn_sort_dev(st["full"], P)
    st["neutral"], ps["neutral"] = rfx.reduce_neutralize(st["full_sort"], ps["full_sort"], cp)
    return st, ps


def chain_equals_model(rfx, rows_s, rows_l, meta, tag):
    want, wps = R.run_stages(rows_s, rows_l, meta["k1"], meta["k2"], meta["P"])
    got, gps = chain(rfx, rows_s, rows_l, meta)
    for s in R.STAGES:
        equals(rfx, got[s], want[s], (tag, s))
    for s in wps:
        assert gps[s].cpu().tolist() == wps[s], (tag, s, "partition starts")
    cp = cparams(rfx, meta)
    out = rfx.reduce_run(*upload(lines(rows_s)), *upload(lines(rows_l)), meta["P"], cp)
    equals(rfx, out, want["neutral"], (tag, "run"))
    assert text_of(rfx, out, meta["k1"]) == R.to_text(want["neutral"], meta["k1"])
    assert text_of(rfx, out, meta["k2"]) == R.to_text(want["neutral"], meta["k2"])


# ---- 1. every operator against the reference's classes -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", case_names(twins=False))
def test_every_operator_equals_its_stage_of_the_reference(rfx, vec, case):
    """each operator is fed the reference's previous output (packed by rfx_dev_dyn_pack) and the reference's partition starts; the
    three sorts are rfx_dev_dyn_sort with the case's P and must give the reference's order and cuts on this stage's mixed-length keys"""
    meta, rs, rl, st, ps, t1, t2 = vec[case]
    cp, P = cparams(rfx, meta), meta["P"]
    equals(rfx, rfx.reduce_union(*upload(lines(rs)), *upload(lines(rl)), cp), st["union"], (case, "union"))
    pk = lambda s: rfx.dyn_pack(host(st[s]))                                                # noqa: E731
    equals(rfx, rfx.reduce_left_prepare(pk("union"), cp), st["left_prep"], (case, "left_prep"))
    for src, dst in (("left_prep", "left_sort"), ("right_prep", "right_sort"), ("full", "full_sort")):
        g, gps = rfx.dyn_sort_dev(pk(src), P)
        equals(rfx, g, st[dst], (case, dst))
        assert gps.cpu().tolist() == ps[dst], (case, dst, "partition starts")
    for src, dst, right in (("left_sort", "left_adj", False), ("right_sort", "right_adj", True)):
        d = pk(src)
        g, gps = rfx.reduce_adjust(d, right, dev_starts(ps[src]), cp)
        equals(rfx, g, st[dst], (case, dst))
        assert gps.cpu().tolist() == ps[dst] and g.n <= d.n, (case, dst, "partition starts, capacity bound")
    equals(rfx, rfx.reduce_right_prepare(pk("left_adj"), cp), st["right_prep"], (case, "right_prep"))
    full = rfx.reduce_full_kmers(pk("right_adj"), cp)
    equals(rfx, full, st["full"], (case, "full"))
    assert full.words == 0
    g, gps = rfx.reduce_neutralize(pk("full_sort"), dev_starts(ps["full_sort"]), cp)
    equals(rfx, g, st["neutral"], (case, "neutral"))
    assert gps.cpu().tolist() == ps["neutral"]
    assert text_of(rfx, g, meta["k1"]) == t1 and text_of(rfx, g, meta["k2"]) == t2, (case, "texts")


@pytest.mark.parametrize("case", case_names())
def test_the_resident_chain_and_the_host_form_equal_both_final_texts(rfx, vec, case):
    meta, rs, rl, st, ps, t1, t2 = vec[case]
    cp = cparams(rfx, meta)
    out = rfx.reduce_run(*upload(lines(rs)), *upload(lines(rl)), meta["P"], cp)
    equals(rfx, out, st["neutral"], (case, "run"))
    assert text_of(rfx, out, meta["k1"]) == t1 and text_of(rfx, out, meta["k2"]) == t2
    g1, g2 = rfx.reduce_text("".join(lines(rs)).encode(), "".join(lines(rl)).encode(), meta["P"], cp)
    assert (g1.decode(), g2.decode()) == (t1, t2)
    assert rfx.last_call_ms > 0


@pytest.mark.parametrize("pair", [(31, 32), (32, 63), (62, 94), (93, 124)])
def test_pairs_where_k_or_k_minus_1_is_a_multiple_of_31(rfx, pair):
    """the reference's classes are sound there (`probe_k` of the vector file), so these pairs are supported: against the model"""
    rs, rl = crafted_rows(np.random.default_rng(pair[0]), *pair)
    chain_equals_model(rfx, rs, rl, dict(k1=pair[0], k2=pair[1], max_k=pair[1], P=3), pair)


# ---- 2. row counts around the block size, against the model --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 255, 256, 257, 511, 512, 513, 3000])
def test_row_counts_around_the_block_size(rfx, vec, n):
    """the first n rows of each input of k31_41_P63 (tiled for 3000 -- duplicates make runs of equal keys): the window filling, a
    pending pair straddling one and two block edges; every stage of the chain, the resident chain and both texts"""
    meta, rs, rl, _, _, _, _ = vec["k31_41_P63"]
    rs, rl = (rs * 14)[:n], (rl * 14)[:n]
    chain_equals_model(rfx, rs, rl, dict(meta, P=2), n)


# ---- 3. two rows pending across block edges -------------------------------------------------------------------------------------------
def long_run(rng, k1, k2, n_long, short_at, right):
    """n_long sub-k-mer rows of k2 - 1 bases in sorted order and (short_at >= 0) one row of k1 - 1 bases, a prefix of the long row
    behind it, put in ahead of that row"""
    keys = sorted({rand_seq(rng, k2 - 1) for _ in range(n_long + 50)}, key=R.block_key)[:n_long]
    recs = [(key, "ACGT"[int(rng.integers(0, 4))], 2 if right else 1, int(rng.choice(MARK)), int(rng.choice(MARK))) for key in keys]
    if short_at >= 0:
        recs.insert(short_at, (recs[short_at][0][:k1 - 1], "ACGT"[int(rng.integers(0, 4))], 2 if right else 1, -1, -1))
    return recs


@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("short_at", [-1, 254, 255, 256, 257, 258])
def test_a_run_of_1200_long_rows_keeps_two_rows_pending_across_four_blocks(rfx, right, short_at):
    """three long rows in a row always shift (:2161-2166): the state is 2 from row 2 to the end, over four block aggregates; one short
    row at 254..258 puts the one decision of the set on either side of the first block edge.  P = 1, and P = 3 cut on a block edge and
    one row past it"""
    k1, k2 = 31, 41
    recs = long_run(np.random.default_rng(7 + short_at), k1, k2, 1200, short_at, right)
    cp = rfx.reduce_params(k1, k2)
    d = rfx.dyn_pack(host(recs))
    for ps in ([0, len(recs)], [0, 256, 513, len(recs)]):
        want, _, wps = R.by_partition(lambda r: R.adjust(r, right, k1), recs, len(ps) - 1, ps)
        g, gps = rfx.reduce_adjust(d, right, dev_starts(ps), cp)
        equals(rfx, g, want, (right, short_at, ps))
        assert gps.cpu().tolist() == wps
        if short_at < 0:
            assert len(want) == len(recs)


@pytest.mark.parametrize("right", [False, True])
def test_partitions_of_0_to_3_rows_and_starts_on_and_past_a_block_edge(rfx, vec, right):
    """the flush at every partition end: partitions of 0, 1, 2 and 3 rows at the front, at a block edge and at the end, a start on
    row 256 and one on row 257; the rows are the case's sorted set, where short and long rows mix"""
    meta, rs, rl, st, _, _, _ = vec["k23_31_P1"]
    recs = st["right_sort" if right else "left_sort"]
    n = len(recs)
    assert n > 300
    ps = [0, 0, 1, 3, 6, 6, 253, 256, 257, 259, n - 6, n - 3, n - 1, n, n]
    want, _, wps = R.by_partition(lambda r: R.adjust(r, right, meta["k1"]), recs, len(ps) - 1, ps)
    g, gps = rfx.reduce_adjust(rfx.dyn_pack(host(recs)), right, dev_starts(ps), cparams(rfx, meta))
    equals(rfx, g, want, ("small partitions", right))
    assert gps.cpu().tolist() == wps
    # 63 partitions, the first 62 of one row each: nothing is compared there, every row comes back
    recs = recs[:300]
    ps = list(range(63)) + [len(recs)]
    want, _, wps = R.by_partition(lambda r: R.adjust(r, right, meta["k1"]), recs, 63, ps)
    assert want[:62] == recs[:62]
    g, gps = rfx.reduce_adjust(rfx.dyn_pack(host(recs)), right, dev_starts(ps), cparams(rfx, meta))
    equals(rfx, g, want, ("63 partitions", right))
    assert gps.cpu().tolist() == wps


def test_the_neutralizers_drop_stretch_across_a_block_edge(rfx, vec):
    """a k2-mer on row 240, then its k1-prefix 40 times (rows 241..280, over the edge at 256): all dropped; with one k1-mer that is
    no prefix on row 262 the stretch ends there and the rows behind it stay; a partition start inside the stretch resets it; a k1-mer
    directly ahead of a k2-mer it is a prefix of is replaced"""
    k1, k2 = 31, 41
    rng = np.random.default_rng(11)
    cp = rfx.reduce_params(k1, k2)
    longs = sorted({rand_seq(rng, k2) for _ in range(400)}, key=R.block_key)
    base = [(s, "", 1, int(rng.choice(MARK)), int(rng.choice(MARK))) for s in longs]
    for variant in ("all", "breaker", "cut", "replaced"):
        recs = list(base)
        stretch = [(recs[240][0][:k1], "", 1, int(rng.choice(MARK)), j) for j in range(40)]
        if variant == "breaker":
            stretch[21] = (rand_seq(rng, k1), "", 1, 5, 5)
        recs[241:241] = stretch
        if variant == "replaced":
            recs.insert(100, (recs[100][0][:k1], "", 1, 9, 9))
        ps = [0, 270, len(recs)] if variant == "cut" else [0, len(recs)]
        want, _, wps = R.by_partition(R.neutralize, recs, len(ps) - 1, ps)
        assert len(want) == len(recs) - {"all": 40, "breaker": 21, "cut": 29, "replaced": 41}[variant], variant
        g, gps = rfx.reduce_neutralize(rfx.dyn_pack(host(recs)), dev_starts(ps), cp)
        equals(rfx, g, want, ("drop stretch", variant))
        assert gps.cpu().tolist() == wps


# ---- 4. contracts --------------------------------------------------------------------------------------------------------------------
def thunks(rfx, vec):
    """every entry point with a packed output, as thunks (params, output struct, P) -> status, on the stages of k33_34_P1"""
    import torch
    meta, rs, rl, st, ps, t1, t2 = vec["k33_34_P1"]
    L, ctx = rfx.L, rfx.ctx
    ds, dl = upload(lines(rs)), upload(lines(rl))
    sets = {s: rfx.dyn_pack(host(st[s])) for s in ("union", "left_sort", "left_adj", "right_sort", "right_adj", "full_sort")}
    ci = {s: d._c() for s, d in sets.items()}
    starts = {s: dev_starts(ps[s]) for s in ("left_sort", "right_sort", "full_sort")}
    ops_out = torch.full((65,), -77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    keep = (ds, dl, sets, ci, starts, ops_out)
    txt = (ds[0].data_ptr(), ds[1].data_ptr(), len(rs), dl[0].data_ptr(), dl[1].data_ptr(), len(rl))
    ops = {
        "union": lambda cp, co, P=1: L.rfx_dev_reduce_union(ctx, *txt, C.byref(cp), C.byref(co)),
        "left_prepare": lambda cp, co, P=1: L.rfx_dev_reduce_left_prepare(ctx, C.byref(ci["union"]), C.byref(cp), C.byref(co)),
        "adjust 0": lambda cp, co, P=1: L.rfx_dev_reduce_adjust(ctx, 0, C.byref(ci["left_sort"]), starts["left_sort"].data_ptr(), P, C.byref(cp), C.byref(co),
                                                              ops_out.data_ptr()),
        "right_prepare": lambda cp, co, P=1: L.rfx_dev_reduce_right_prepare(ctx, C.byref(ci["left_adj"]), C.byref(cp), C.byref(co)),
        "adjust 1": lambda cp, co, P=1: L.rfx_dev_reduce_adjust(ctx, 1, C.byref(ci["right_sort"]), starts["right_sort"].data_ptr(), P, C.byref(cp), C.byref(co),
                                                              ops_out.data_ptr()),
        "full_kmers": lambda cp, co, P=1: L.rfx_dev_reduce_full_kmers(ctx, C.byref(ci["right_adj"]), C.byref(cp), C.byref(co)),
        "neutralize": lambda cp, co, P=1: L.rfx_dev_reduce_neutralize(ctx, C.byref(ci["full_sort"]), starts["full_sort"].data_ptr(), P, C.byref(cp), C.byref(co),
                                                                    ops_out.data_ptr()),
        "run": lambda cp, co, P=1: L.rfx_dev_reduce_run(ctx, *txt, P, C.byref(cp), C.byref(co)),
    }
    return meta, rs, rl, ops, keep


@pytest.mark.parametrize("pair", [(33, 33), (34, 33), (7, 34), (33, 125), (0, 0)])
def test_a_refused_pair_returns_the_code_and_writes_nothing(rfx, vec, pair):
    meta, rs, rl, ops, keep = thunks(rfx, vec)
    cp = rfx.reduce_params(*pair)
    n = len(rs) + len(rl)
    for name, call in ops.items():
        d = poisoned(n, n)
        co = d._c()
        co.n = co.need_words = -77
        assert call(cp, co) == E_ARG, (name, pair)
        assert untouched(d) and (int(co.n), int(co.need_words)) == (-77, -77), (name, pair)
    assert bool((keep[5] == -77).all())
    cp = rfx.reduce_params(33, 34, max_k=33)                       # the last k of the list below k2
    assert ops["run"](cp, poisoned(n, n)._c()) == E_ARG
    o1, o2, l1, l2 = np.full(64, FILL, np.uint8), np.full(64, FILL, np.uint8), C.c_int64(-77), C.c_int64(-77)
    off = np.array([0, 14], np.int64)
    cp = rfx.reduce_params(*pair)
    assert rfx.L.rfx_reduce_text(rfx.ctx, b"ACGTACGT,1|2|3", off.ctypes.data, 1, b"ACGTACGT,1|2|3", off.ctypes.data, 1, 1, C.byref(cp), o1.ctypes.data, 64,
                                 C.addressof(l1), o2.ctypes.data, 64, C.addressof(l2)) == E_ARG
    assert (l1.value, l2.value) == (-77, -77) and (o1 == FILL).all() and (o2 == FILL).all()


def test_bad_partition_counts_null_pointers_bad_starts_and_a_third_key_length(rfx, vec):
    meta, rs, rl, ops, keep = thunks(rfx, vec)
    cp = cparams(rfx, meta)
    n = len(rs) + len(rl)
    ds, dl, sets, ci, starts, ops_out = keep
    L, ctx = rfx.L, rfx.ctx
    d = poisoned(n, n)
    for P in (0, 64, -1):
        for name in ("adjust 0", "adjust 1", "neutralize", "run"):
            assert ops[name](cp, d._c(), P) == E_ARG, (name, P)
    o1, o2, l1, l2 = np.full(64, FILL, np.uint8), np.full(64, FILL, np.uint8), C.c_int64(-77), C.c_int64(-77)
    off = np.array([0, 14], np.int64)
    for P in (0, 64):
        assert L.rfx_reduce_text(ctx, b"ACGTACGT,1|2|3", off.ctypes.data, 1, b"ACGTACGT,1|2|3", off.ctypes.data, 1, P, C.byref(cp), o1.ctypes.data, 64,
                                 C.addressof(l1), o2.ctypes.data, 64, C.addressof(l2)) == E_ARG
    # null pointers
    txt = (ds[0].data_ptr(), ds[1].data_ptr(), len(rs), dl[0].data_ptr(), dl[1].data_ptr(), len(rl))
    assert L.rfx_dev_reduce_union(ctx, None, txt[1], txt[2], txt[3], txt[4], txt[5], C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_reduce_union(ctx, txt[0], txt[1], txt[2], txt[3], None, txt[5], C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_reduce_union(ctx, *txt, None, C.byref(d._c())) == E_ARG
    assert L.rfx_dev_reduce_run(ctx, *txt, 1, C.byref(cp), None) == E_ARG
    assert L.rfx_dev_reduce_left_prepare(ctx, None, C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_reduce_right_prepare(ctx, C.byref(ci["left_adj"]), C.byref(cp), None) == E_ARG
    assert L.rfx_dev_reduce_full_kmers(ctx, C.byref(ci["right_adj"]), None, C.byref(d._c())) == E_ARG
    assert L.rfx_dev_reduce_adjust(ctx, 0, C.byref(ci["left_sort"]), None, 1, C.byref(cp), C.byref(d._c()), ops_out.data_ptr()) == E_ARG
    assert L.rfx_dev_reduce_adjust(ctx, 0, C.byref(ci["left_sort"]), starts["left_sort"].data_ptr(), 1, C.byref(cp), C.byref(d._c()), None) == E_ARG
    assert L.rfx_dev_reduce_adjust(ctx, 2, C.byref(ci["left_sort"]), starts["left_sort"].data_ptr(), 1, C.byref(cp), C.byref(d._c()), ops_out.data_ptr()) == E_ARG
    assert L.rfx_dev_reduce_neutralize(ctx, C.byref(ci["full_sort"]), None, 1, C.byref(cp), C.byref(d._c()), ops_out.data_ptr()) == E_ARG
    no_key = d._c()
    no_key.key = None
    assert L.rfx_dev_reduce_left_prepare(ctx, C.byref(ci["union"]), C.byref(cp), C.byref(no_key)) == E_ARG
    # partition starts that do not run from 0 to n
    m = sets["left_sort"].n
    for bad in ([1, m], [0, m - 1], [0, m + 1], [0, 9, 5, m]):
        t = dev_starts(bad)
        assert L.rfx_dev_reduce_adjust(ctx, 0, C.byref(ci["left_sort"]), t.data_ptr(), len(bad) - 1, C.byref(cp), C.byref(d._c()), ops_out.data_ptr()) == E_ARG, bad
    m = sets["full_sort"].n
    for bad in ([1, m], [0, m + 1], [0, 9, 5, m]):
        t = dev_starts(bad)
        assert L.rfx_dev_reduce_neutralize(ctx, C.byref(ci["full_sort"]), t.data_ptr(), len(bad) - 1, C.byref(cp), C.byref(d._c()), ops_out.data_ptr()) == E_ARG, bad
    # a set with a third key length; a set whose extensions are not what the operator reads
    k1, k2 = meta["k1"], meta["k2"]
    sub = lambda ln, e="C": (rand_seq(np.random.default_rng(ln), ln), e, 1, 3, 3)                     # noqa: E731
    third_sub = rfx.dyn_pack(host([sub(k1 - 1), sub(k2 - 1), sub(k2)]))
    third_full = rfx.dyn_pack(host([sub(k1, ""), sub(k2, ""), sub(k2 + 1, "")]))
    long_ext = rfx.dyn_pack(host([sub(k1 - 1, "CC"), sub(k2 - 1)]))
    no_ext = rfx.dyn_pack(host([sub(k1 - 1, ""), sub(k2 - 1, "")]))
    t3, t2 = dev_starts([0, 3]), dev_starts([0, 2])
    for pk, t in ((third_sub, t3), (long_ext, t2), (no_ext, t2)):
        c = pk._c()
        assert L.rfx_dev_reduce_adjust(ctx, 0, C.byref(c), t.data_ptr(), 1, C.byref(cp), C.byref(d._c()), ops_out.data_ptr()) == E_ARG
        assert L.rfx_dev_reduce_adjust(ctx, 1, C.byref(c), t.data_ptr(), 1, C.byref(cp), C.byref(d._c()), ops_out.data_ptr()) == E_ARG
        assert L.rfx_dev_reduce_right_prepare(ctx, C.byref(c), C.byref(cp), C.byref(d._c())) == E_ARG
        assert L.rfx_dev_reduce_full_kmers(ctx, C.byref(c), C.byref(cp), C.byref(d._c())) == E_ARG
    for pk, t in ((third_full, t3), (third_sub, t3), (long_ext, t2)):
        c = pk._c()
        assert L.rfx_dev_reduce_left_prepare(ctx, C.byref(c), C.byref(cp), C.byref(d._c())) == E_ARG
        assert L.rfx_dev_reduce_neutralize(ctx, C.byref(c), t.data_ptr(), 1, C.byref(cp), C.byref(d._c()), ops_out.data_ptr()) == E_ARG
    # a row without a comma
    bad_rows = upload(["ACGTACGTACGTACGTACGTACGTACGTACGTA 1|2|3\n"])
    assert L.rfx_dev_reduce_union(ctx, bad_rows[0].data_ptr(), bad_rows[1].data_ptr(), 1, txt[3], txt[4], txt[5], C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_reduce_run(ctx, txt[0], txt[1], txt[2], bad_rows[0].data_ptr(), bad_rows[1].data_ptr(), 1, 1, C.byref(cp), C.byref(d._c())) == E_ARG
    assert untouched(d) and bool((ops_out == -77).all())
    assert (l1.value, l2.value) == (-77, -77) and (o1 == FILL).all() and (o2 == FILL).all()


def test_every_capacity_one_short(rfx, vec):
    """cap_n = need - 1, then cap_words = need - 1: RFX_E_CAP with n / need_words set, every output tensor (0xA5) and the output
    partition starts as they were; with exactly the needs the same call succeeds.  The sets of full k-mers need no extension words"""
    meta, rs, rl, ops, keep = thunks(rfx, vec)
    cp = cparams(rfx, meta)
    n = len(rs) + len(rl)
    for name, call in ops.items():
        big = poisoned(n, n)
        co = big._c()
        assert call(cp, co) == OK, name
        need_n, need_w = int(co.n), int(co.need_words)
        assert 0 < need_n <= n and need_w == (0 if name in ("union", "full_kmers", "neutralize", "run") else need_n), (name, need_n, need_w)
        exact = poisoned(need_n, need_w)
        assert call(cp, exact._c()) == OK and not untouched(exact), name
        keep[5].fill_(-77)
        for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
            if cap_w < 0:
                continue
            d = poisoned(cap_n, cap_w)
            co = d._c()
            co.n = co.need_words = -77
            assert call(cp, co) == E_CAP, (name, cap_n, cap_w)
            assert (int(co.n), int(co.need_words)) == (need_n, need_w), name
            assert untouched(d) and bool((keep[5] == -77).all()), (name, cap_n, cap_w)


def test_text_buffers_one_byte_short(rfx, vec):
    """rfx_reduce_text with either buffer one byte short: RFX_E_CAP, both lengths, neither buffer written; rfx_dev_ksort_to_text of the
    final set with cap = length - 1 follows the text-buffer rule"""
    import torch
    meta, rs, rl, st, ps, t1, t2 = vec["k33_34_P1"]
    cp = cparams(rfx, meta)
    ts, tl = "".join(lines(rs)).encode(), "".join(lines(rl)).encode()
    offs, ns = rfx._row_offsets(ts)
    offl, nl = rfx._row_offsets(tl)
    n1, n2 = len(t1), len(t2)
    for c1, c2 in ((n1 - 1, n2), (n1, n2 - 1), (0, 0)):
        o1, o2, l1, l2 = np.full(n1 + 16, FILL, np.uint8), np.full(n2 + 16, FILL, np.uint8), C.c_int64(0), C.c_int64(0)
        assert rfx.L.rfx_reduce_text(rfx.ctx, ts, offs.ctypes.data, ns, tl, offl.ctypes.data, nl, 1, C.byref(cp), o1.ctypes.data, c1, C.addressof(l1),
                                     o2.ctypes.data, c2, C.addressof(l2)) == E_CAP
        assert (l1.value, l2.value) == (n1, n2) and (o1 == FILL).all() and (o2 == FILL).all()
    o1, o2, l1, l2 = np.full(n1 + 16, FILL, np.uint8), np.full(n2 + 16, FILL, np.uint8), C.c_int64(0), C.c_int64(0)
    assert rfx.L.rfx_reduce_text(rfx.ctx, ts, offs.ctypes.data, ns, tl, offl.ctypes.data, nl, 1, C.byref(cp), o1.ctypes.data, n1, C.addressof(l1),
                                 o2.ctypes.data, n2, C.addressof(l2)) == OK
    assert o1[:n1].tobytes().decode() == t1 and o2[:n2].tobytes().decode() == t2 and (o1[n1:] == FILL).all() and (o2[n2:] == FILL).all()
    pk = rfx.dyn_pack(host(st["neutral"]))
    ci = pk._c()
    d_text = torch.full((n2 + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ln, nr = C.c_int64(0), C.c_int64(0)
    assert rfx.L.rfx_dev_ksort_to_text(rfx.ctx, C.byref(ci), meta["k2"], d_text.data_ptr(), n2 - 1, C.addressof(ln), None, C.addressof(nr)) == E_CAP
    assert ln.value == n2 and bool((d_text[n2 - 1:] == FILL).all()) and bytes(d_text[:n2 - 1].cpu().numpy()).decode() == t2[:-1]


def test_an_empty_input_through_every_entry_point(rfx):
    cp = rfx.reduce_params(31, 41)
    none, one = upload([]), upload(["ACGT,1|2|3\n"])                 # (a row of another length: dropped)
    u = rfx.reduce_union(*none, *none, cp)
    assert u.n == 0
    lp = rfx.reduce_left_prepare(u, cp)
    s, ps = rfx.dyn_sort_dev(lp, 5)
    a0, ps0 = rfx.reduce_adjust(s, False, ps, cp)
    a1, ps1 = rfx.reduce_adjust(s, True, ps, cp)
    nt, ps2 = rfx.reduce_neutralize(u, ps, cp)
    outs = [u, lp, a0, a1, rfx.reduce_right_prepare(a0, cp), rfx.reduce_full_kmers(a1, cp), nt, rfx.reduce_run(*none, *none, 5, cp),
            rfx.reduce_run(*one, *none, 1, cp), rfx.reduce_union(*none, *one, cp)]
    for t in outs:
        assert t.n == 0 and int(t.ext_off[0]) == 0
    for t in (ps0, ps1, ps2):
        assert t.cpu().tolist() == [0] * 6
    assert rfx.reduce_text(b"", b"", 3, cp) == (b"", b"")
    # one input empty: the other goes through (nothing to compare it with)
    rng = np.random.default_rng(3)
    rows = [f"{rand_seq(rng, 41)},1|{j}|-1\n" for j in range(5)]
    g1, g2 = rfx.reduce_text(b"", "".join(rows).encode(), 2, cp)
    assert (g1.decode(), g2.decode()) == R.run_text([], rows, 31, 41, 2) and g1 == b"" and g2.count(b"\n") == 5


# ---- 5. the hand-over in and out ------------------------------------------------------------------------------------------------------
def test_two_texts_of_the_sorting_stage_feed_the_stage_directly(rfx):
    """rfx_dev_ksort_run + rfx_dev_ksort_to_text at k = 31 and k = 33 (two cases of tests/golden/ksort_vectors.npz): d_text and
    d_row_off of both go straight into rfx_dev_reduce_run"""
    from tests import ksort_model as K
    z = np.load(os.path.join(os.path.dirname(VEC), "ksort_vectors.npz"))
    texts, dev = [], []
    for name in ("k31_m97", "k33_m97"):
        p, rows, st, text = K.load_case(z, name)
        out = rfx.ksort_run(*upload(rows), rfx.ksort_params(p["k"], max_k=p["max_k"]))
        d_text, ln, d_off, n = rfx.ksort_to_text_dev(out, p["k"])
        assert bytes(d_text[:ln].cpu().numpy()).decode() == text
        texts.append(text.splitlines(True))
        dev += [d_text[:ln], d_off[:n + 1]]
    cp = rfx.reduce_params(31, 33, max_k=97)
    out = rfx.reduce_run(*dev, 4, cp)
    w1, w2 = R.run_text(texts[0], texts[1], 31, 33, 4)
    assert text_of(rfx, out, 31) == w1 and text_of(rfx, out, 33) == w2 and len(w1) > 0 and len(w2) > 0


@pytest.mark.parametrize("case", ["k31_41_P63", "k64_65_P7", "k97_124_P1"])
def test_the_texts_and_their_row_offsets_go_straight_to_the_dynamic_k_binarizer(rfx, vec, case):
    """d_text and d_row_off of rfx_dev_ksort_to_text on the stage's final set -> rfx_dev_dyn_binarize form 0 -> rfx_dev_dyn_sort"""
    meta, rs, rl, st, ps, t1, t2 = vec[case]
    out = rfx.reduce_run(*upload(lines(rs)), *upload(lines(rl)), meta["P"], cparams(rfx, meta))
    for k, text in ((meta["k1"], t1), (meta["k2"], t2)):
        d_text, ln, d_off, n = rfx.ksort_to_text_dev(out, k)
        pk = rfx.dyn_binarize_dev(d_text[:ln], d_off[:n + 1], 0)
        want = R.handover(text)
        assert len(want) == n
        equals(rfx, pk, want, (case, k, "hand-over"))
        s, sps = rfx.dyn_sort_dev(pk, 4)
        equals(rfx, s, R.sort_records(want), (case, k, "hand-over, sorted"))
        assert sps.cpu().tolist()[0] == 0 and sps.cpu().tolist()[-1] == n


def test_reflexiv_host_reduce_in_pair_form_writes_both_texts_under_the_right_names(vec, tmp_path):
    """`reflexiv_host reduce -kmerc SHORT -kmerc2 LONG -kmer K1 -kmer2 K2 -klist ... -partition P -outfile O` ->
    O/Count_K1_reduced/part-00000.csv and O/Count_K2_sorted/..., or O/Count_K2_reduced/... when K2 is the last k of the list"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reflexiv_amd", "reflexiv_host")
    for case, klist, second in (("k31_41_P63", "23,31,41", "reduced"), ("k31_41_P63", "31,41,53", "sorted"), ("k64_65_P7", "64,65,95", "sorted")):
        meta, rs, rl, st, ps, t1, t2 = vec[case]
        a, b, out = tmp_path / "short.csv", tmp_path / "long.csv", tmp_path / (case + second)
        a.write_text("".join(lines(rs)))
        b.write_text("".join(lines(rl)))
        r = subprocess.run([exe, "reduce", "-kmerc", str(a), "-kmerc2", str(b), "-kmer", str(meta["k1"]), "-kmer2", str(meta["k2"]), "-klist", klist,
                            "-partition", str(meta["P"]), "-outfile", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert (out / f"Count_{meta['k1']}_reduced" / "part-00000.csv").read_text() == t1, case
        assert (out / f"Count_{meta['k2']}_{second}" / "part-00000.csv").read_text() == t2, case
        assert (out / f"Count_{meta['k2']}_{second}" / "_SUCCESS").exists()
        assert not (out / f"Count_{meta['k2']}_{'sorted' if second == 'reduced' else 'reduced'}").exists()
    r = subprocess.run([exe, "reduce", "-kmerc", str(a), "-kmerc2", str(b), "-kmer", "41", "-kmer2", "31", "-outfile", str(tmp_path / "x")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "41" in r.stderr


def test_reflexiv_host_reduce_in_list_form_equals_the_pairs_run_by_hand(rfx, tmp_path):
    """-kmerc DIR -klist 23,31,33: DIR/Count_<k> of every k through the sorting stage, then (23, 31) and (31, 33), the second pair
    reading the first pair's rewritten Count_31_sorted"""
    import subprocess
    from tests import ksort_model as K
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reflexiv_amd", "reflexiv_host")
    z = np.load(os.path.join(os.path.dirname(VEC), "ksort_vectors.npz"))
    src, out, texts = tmp_path / "counts", tmp_path / "out", {}
    src.mkdir()
    for k in (23, 31, 33):
        p, rows, st, text = K.load_case(z, f"k{k}_m97")
        (src / f"Count_{k}").mkdir()
        (src / f"Count_{k}" / "part-00000.csv").write_text("".join(rows))
        texts[k] = rfx.ksort_text("".join(rows).encode(), rfx.ksort_params(k, max_k=33))
    r23, s31 = rfx.reduce_text(texts[23], texts[31], 5, rfx.reduce_params(23, 31, max_k=33))
    r31, r33 = rfx.reduce_text(s31, texts[33], 5, rfx.reduce_params(31, 33, max_k=33))
    assert len(r23) and len(r31) and len(r33) and s31 != texts[31]
    r = subprocess.run([exe, "reduce", "-kmerc", str(src), "-klist", "23,31,33", "-partition", "5", "-outfile", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name, want in (("Count_23_reduced", r23), ("Count_31_sorted", s31), ("Count_31_reduced", r31), ("Count_33_reduced", r33)):
        assert (out / name / "part-00000.csv").read_bytes() == want, name


# ---- 6. poisoned allocations ---------------------------------------------------------------------------------------------------------
def test_the_stage_holds_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it, so a producer that
    relied on zeroed memory for its padding bits or unused key words fails the raw-word checks above.  A child process: the mask is
    read once per process."""
    import subprocess
    import sys
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
