"""The dynamic-k passes on the PACKED record set that stays in HBM (rfx_dev_dyn_*, rfx_dyn_run_text):
pack / unpack against a numpy packer (raw words, zero padding bits, zero unused key words), every operator against the rows the
reference's own classes made (tests/golden/dynamic_vectors.npz c0..c4, dynamic_edge_vectors.npz e0..e3), the resident chain text
to text, every shift of the word-wise concatenation against the oracle, the capacity / limit / argument contracts, and all of it
again with every allocation poisoned.  The checkers are the existing ones: the reference-made vectors, oracle.dyn_* and the
string model tests/pymodel.py."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import pymodel as M
from tests.test_oracle_dynamic import VEC, EDGE, cases, edge_cases, rows_of, model_rows
from tests.test_gpu_dynamic_edges import same_records, same_rows

pytestmark = pytest.mark.gpu

OK, E_ARG, E_CAP, E_LIMIT = 0, -1, -2, -6
FILL = 0xA5
NUC = "ACGT"
KEY_LENGTHS = (1, 22, 31, 32, 33, 62, 63, 64, 65, 93, 96, 97, 124)
EXT_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 1000)


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


# ---- a numpy statement of the layout ----------------------------------------------------------------------------------------------
def words_of(codes):
    """base codes -> 64-bit words, 32 bases each, the first in the two highest bits, 0 behind the last base"""
    nw = (len(codes) + 31) // 32
    c = np.zeros(nw * 32, np.uint64)
    c[:len(codes)] = codes
    return np.bitwise_or.reduce(c.reshape(nw, 32) << (np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)), axis=1) if nw else np.zeros(0, np.uint64)


def np_packed(r):
    """a DynRecords (device or oracle form) -> (key [n, 4], key_len, ext words, ext_off in words, ext_len)"""
    n = r.n
    key = np.zeros((n, 4), np.uint64)
    ext, ext_off = [], np.zeros(n + 1, np.int64)
    for i in range(n):
        w = words_of(np.asarray(r.key[r.key_off[i]:r.key_off[i + 1]]))
        key[i, :len(w)] = w
        e = words_of(np.asarray(r.ext[r.ext_off[i]:r.ext_off[i + 1]]))
        ext.append(e)
        ext_off[i + 1] = ext_off[i] + len(e)
    return (key, np.diff(r.key_off[:n + 1]).astype(np.uint8), np.concatenate(ext) if ext else np.zeros(0, np.uint64), ext_off,
            np.diff(r.ext_off[:n + 1]).astype(np.int32))


def raw_equals(pk, r, tag):
    """the words in HBM are the numpy packer's of record set r: bases, zero padding bits, zero unused key words, offsets, lengths,
    attributes"""
    key, key_len, ext, ext_off, ext_len, marker, left, right = pk.host()
    wk, wkl, we, weo, wel = np_packed(r)
    for name, a, b in (("key", key, wk), ("key_len", key_len, wkl), ("ext_off", ext_off, weo), ("ext_len", ext_len, wel), ("ext", ext, we),
                       ("marker", marker, r.marker[:r.n]), ("left", left, r.left[:r.n]), ("right", right, r.right[:r.n])):
        assert a.shape == b.shape and np.array_equal(a, b), (tag, name, a.shape, b.shape)


def padding_is_zero(rfx, pk, tag):
    """the invariant on the raw words: the set unpacked and packed again by numpy gives the same words -> the unpacked set"""
    r = rfx.dyn_unpack(pk)
    raw_equals(pk, r, (tag, "padding"))
    return r


def records_of(rng, n):
    """n records over every (key length, extension length) of the lists (13 and 9 are coprime), bases 0..3, both markers"""
    from reflexiv_amd.api import DynRecords
    rnd = lambda m: "".join(NUC[b] for b in rng.integers(0, 4, m))
    return DynRecords.from_text([rnd(KEY_LENGTHS[i % 13]) for i in range(n)], [rnd(EXT_LENGTHS[i % 9]) for i in range(n)],
                                [1 + i % 2 for i in range(n)], [int(rng.integers(-50, 50)) for _ in range(n)],
                                [int(rng.integers(-50, 50)) for _ in range(n)])


# ---- 1. pack / unpack and the raw words ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_pack_and_unpack_against_a_numpy_packer(rfx, n):
    """keys of 1..124 bases around every word and block edge, extensions of 0..1000 bases, code 3 included: the words, lengths and
    offsets in HBM are the numpy packer's (so every padding bit and every unused key word is 0), and unpack(pack(x)) = x"""
    r = records_of(np.random.default_rng(60 + n), n)
    if n >= 255:
        assert {(int(a), int(b)) for a, b in zip(np.diff(r.key_off), np.diff(r.ext_off))} == {(a, b) for a in KEY_LENGTHS for b in EXT_LENGTHS}
        assert 3 in r.key and 3 in r.ext
    pk = rfx.dyn_pack(r)
    assert pk.n == n
    raw_equals(pk, r, ("pack", n))
    same_records(rfx.dyn_unpack(pk), r, ("unpack", n))


# ---- 2. every operator against the reference's classes --------------------------------------------------------------------------------
def step(rfx, prev_rows, P, stage, start, start_marker, want_rows, tag):
    """pack -> sort -> extend pass -> unpack on the reference's previous output, with the raw-word invariant and the capacity bound
    after each operator"""
    from reflexiv_amd.api import DynRecords
    o = O.dyn_sort(O.dyn_binarize_rows(prev_rows))
    pk = rfx.dyn_pack(DynRecords.from_rows(prev_rows))
    n_in, w_in = pk.n, pk.words
    padding_is_zero(rfx, pk, (tag, "pack"))
    s, ps = rfx.dyn_sort_dev(pk, P)
    same_records(padding_is_zero(rfx, s, (tag, "sort")), o, (tag, "sort"))
    want_ps = O.dyn_partition_starts(o, P)
    assert np.array_equal(ps.cpu().numpy(), want_ps), (tag, "part_start")
    assert s.n == n_in and s.words == w_in
    g, ops = rfx.dyn_extend_pass_dev(s, ps, stage, start, start_marker)
    got = padding_is_zero(rfx, g, (tag, "pass"))
    same_rows(got, want_rows, (tag, "pass"))
    _, want_ops = O.dyn_extend_pass(o, want_ps, stage, start, start_marker)
    assert np.array_equal(ops.cpu().numpy(), want_ops), (tag, "out_part_start")
    assert g.n <= n_in and g.words <= w_in, (tag, "capacity bound", g.n, n_in, g.words, w_in)


@pytest.mark.parametrize("case", cases())
def test_packed_operators_equal_the_reference_classes(rfx, case):
    """c0..c4: the random reflection, the four FirstFour passes and every Iteration pass, each fed the reference's previous output
    (c4 reaches extensions of 761 bases: 24 words)"""
    import torch
    from reflexiv_amd.api import DynRecords
    z = np.load(VEC)
    P, start, end = (int(x) for x in z[case + "/meta"])
    r = DynRecords.from_kmer_rows(rows_of(z, case + "/in"))
    pk = rfx.dyn_pack(r)
    st = torch.tensor([p * r.n // P for p in range(P)] + [r.n], dtype=torch.int64, device="cuda")
    g = rfx.dyn_random_reflection_dev(pk, st)
    same_rows(padding_is_zero(rfx, g, (case, "random reflection")), rows_of(z, case + "/random_reflection"), (case, "random reflection"))
    assert g.n == pk.n and g.words == pk.words
    prev = "random_reflection"
    for it in range(4):
        step(rfx, rows_of(z, f"{case}/{prev}"), P, 0, 5, 2, rows_of(z, f"{case}/extend{it}"), (case, f"extend{it}"))
        prev = f"extend{it}"
    prev = "it_binarized"
    for it in range(start + 1, end + 2):
        step(rfx, rows_of(z, f"{case}/{prev}"), P, 1, start, 2, rows_of(z, f"{case}/it_extend{it}"), (case, f"it_extend{it}"))
        prev = f"it_extend{it}"


@pytest.mark.parametrize("case", edge_cases())
def test_packed_operators_equal_the_reference_classes_on_crafted_families(rfx, case):
    """e0..e3: keys of 22..94 bases at the block edges 31, 32, 61..63, 92, 93, every distance branch, the rules from 61 on"""
    z = np.load(EDGE)
    P, stage, start, start_marker, passes = (int(x) for x in z[case + "/meta"])
    prev = rows_of(z, case + "/in")
    for i in range(passes):
        want = rows_of(z, f"{case}/pass{i}")
        step(rfx, prev, P, stage, start, start_marker, want, (case, i))
        prev = want


# ---- 3. the resident chain, text to text ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases())
def test_run_text_equals_the_reference_files(rfx, case):
    """rfx_dyn_run_text: the bytes of case/in -> the bytes of case/extend3 (FirstFour), those -> case/final (Iteration); and the same
    chain composed from Python on device tensors (binarize -> run -> to-text) gives the same bytes and traces.  (The edge vectors
    hold single passes, no drivers' files: they are in the operator test above.)"""
    import torch
    z = np.load(VEC)
    P, start, end = (int(x) for x in z[case + "/meta"])
    src, ff_want, fin_want = bytes(z[case + "/in"]), bytes(z[case + "/extend3"]), bytes(z[case + "/final"])
    ff, tr_ff = rfx.dyn_run_text(src, 0, P, random_reflection=True, passes_first_four=4)
    assert ff == ff_want, (case, "first four", len(ff), len(ff_want))
    assert tr_ff == [len(rows_of(z, f"{case}/extend{i}")) for i in range(4)]
    fin, tr_it = rfx.dyn_run_text(ff_want, 1, P, start_iteration=start, end_iteration=end)
    assert fin == fin_want, (case, "iterations", len(fin), len(fin_want))
    assert len(tr_it) == end - start + 1 and tr_it[-1] == len(rows_of(z, case + "/final"))

    def composed(text, form, **kw):
        buf = np.frombuffer(text, np.uint8)
        off = np.concatenate([[0], np.flatnonzero(buf == 10) + 1]).astype(np.int64)      # (every line of these files is a row)
        assert off[-1] == len(buf)
        d_text, d_off = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(off).cuda()
        pk = rfx.dyn_binarize_dev(d_text, d_off, form)
        out, tr = rfx.dyn_run_dev(pk, P, **kw)
        assert out.n <= pk.n and out.words <= pk.words
        d_out, ln = rfx.dyn_to_text_dev(out)
        return bytes(d_out[:ln].cpu().numpy()), tr
    assert composed(src, 0, random_reflection=True, passes_first_four=4) == (ff_want, tr_ff)
    assert composed(ff_want, 1, start_iteration=start, end_iteration=end) == (fin_want, tr_it)


# ---- 4. every shift of the word-wise concatenation -------------------------------------------------------------------------------------
SHIFT_SEED = 71


def shift_records(seed=SHIFT_SEED):
    """about 4000 records in families (keys = prefixes of a family string, 20..124 bases; extensions of 0..200 bases; both markers;
    the attributes of the crafted families), and two families of one forward + one reflected row with extensions of 5000 and
    10001 bases: a key of G's sorts among the first and a key of C's among the last (signed blocks), so at P = 2 they lie on
    either side of the cut"""
    rng = np.random.default_rng(seed)
    rnd = lambda m: "".join(NUC[b] for b in rng.integers(0, 4, m))
    recs = []
    while len(recs) < 4000:
        fam = rnd(124)
        for _ in range(int(rng.integers(1, 5))):
            recs.append((fam[:int(rng.integers(20, 125))], int(rng.integers(1, 3)), rnd(int(rng.integers(0, 201))),
                         M.dyn_crafted_attribute(rng), M.dyn_crafted_attribute(rng)))
    for key, ef, er in (("G" * 40, 5000, 10001), ("C" * 95, 10001, 5000)):
        recs += [(key, 1, rnd(ef), -3, -4), (key, 2, rnd(er), -5, -6)]
    return [recs[i] for i in rng.permutation(len(recs))]


def shift_census(monkeypatch, m, starts, stage, start):
    """the string model's pass with its flips and merges recorded -> (flips: (marker, m, |key|, |ext|), merges: (|P|, |L|, |S|))"""
    flips, merges = [], []
    flip, merge = M.dyn_flip, M.dyn_merge
    monkeypatch.setattr(M, "dyn_flip", lambda r, mm: (flips.append((r[1], mm, len(r[0]), len(r[2]))), flip(r, mm))[1])
    monkeypatch.setattr(M, "dyn_merge", lambda F, R, d, mm, lb: (merges.append((len(R[2]), max(len(F[0]), len(R[0])), len(F[2]))),
                                                                 merge(F, R, d, mm, lb))[1])
    out, ostarts, _ = M.dyn_extend_pass(m, starts, stage, start)
    monkeypatch.undo()
    return out, ostarts, flips, merges


@pytest.mark.parametrize("stage,start", [(0, 0), (1, 5)])
def test_every_shift_of_the_word_wise_concatenation(rfx, monkeypatch, stage, start):
    """one pass (stage 0, stage 1) over the set above at P = 2 against the oracle field by field.  Asserted on the CPU first, from
    the string model: among the flips 1 -> 2 and among the flips 2 -> 1 every residue of |ext| mod 32 occurs, among the merges
    every residue of |P| mod 32 and of (|P| + |L|) mod 32, a flip has |ext| > |key|, and the two long families merge (extensions
    of 15001 bases: 469 output words from one record) on either side of the cut."""
    from reflexiv_amd.api import DynRecords
    recs = shift_records()
    assert 4000 <= len(recs) < 4100
    m = M.dyn_sort(recs)
    starts = M.dyn_partition_starts(m, 2)
    out, ostarts, flips, merges = shift_census(monkeypatch, m, starts, stage, start)
    every = set(range(32))
    assert {e % 32 for mk, mm, k, e in flips if (mk, mm) == (1, 2)} == every
    assert {e % 32 for mk, mm, k, e in flips if (mk, mm) == (2, 1)} == every
    assert {p % 32 for p, l, s in merges} == every and {(p + l) % 32 for p, l, s in merges} == every
    assert any(e > k for mk, mm, k, e in flips if mk != mm)
    assert (10001, 40, 5000) in merges and (5000, 95, 10001) in merges
    longest = [i for i, r in enumerate(out) if len(r[2]) == 15001]
    assert len(longest) == 2 and longest[0] < ostarts[1] <= longest[1]
    assert max(i for i, r in enumerate(m) if r[0] == "G" * 40) < starts[1] <= min(i for i, r in enumerate(m) if r[0] == "C" * 95)

    o = O.dyn_sort(O.dyn_binarize_rows(model_rows(recs)))
    pk = rfx.dyn_pack(DynRecords.from_rows(model_rows(recs)))
    s, ps = rfx.dyn_sort_dev(pk, 2)
    want_ps = O.dyn_partition_starts(o, 2)
    assert list(want_ps) == starts and np.array_equal(ps.cpu().numpy(), want_ps)
    same_records(rfx.dyn_unpack(s), o, ("shift", "sort"))
    want, want_ops = O.dyn_extend_pass(o, want_ps, stage, start, 2)
    g, ops = rfx.dyn_extend_pass_dev(s, ps, stage, start, 2)
    got = padding_is_zero(rfx, g, ("shift", stage))
    same_records(got, want, ("shift", stage))
    same_rows(got, model_rows(out), ("shift", stage, "model"))
    assert np.array_equal(ops.cpu().numpy(), want_ops)
    assert g.n <= s.n and g.words <= s.words


# ---- 5. contracts ------------------------------------------------------------------------------------------------------------------------
def poisoned(cap_n, cap_words):
    """an output set whose every tensor is filled with 0xA5"""
    import torch
    from reflexiv_amd.api import DynPacked
    d = DynPacked(cap_n, cap_words)
    for t in d.tensors():
        t.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    return d


def untouched(d):
    import torch
    return all(bool((t.view(torch.uint8) == FILL).all()) for t in d.tensors())


def small_sorted_set(rfx):
    """a packed, sorted set with merges in reach, its part starts (P = 3) and its host form"""
    from reflexiv_amd.api import DynRecords
    recs = M.dyn_crafted_families(np.random.default_rng(81), 40, M.DYN_WIDE_LENGTHS, ext_max=70)
    r = DynRecords.from_rows(model_rows(M.dyn_sort(recs)))
    pk = rfx.dyn_pack(r)
    s, ps = rfx.dyn_sort_dev(pk, 3)
    return r, s, ps


def operators(rfx, r, s, ps, P=3):
    """every entry point with a packed output, as thunks on a given output struct -> status"""
    import torch
    L, ctx = rfx.L, rfx.ctx
    ci, hi = s._c(), r._c()
    text = "".join(",".join(f) + "\n" for f in r.rows()).encode()
    buf = np.frombuffer(text, np.uint8)
    d_text = torch.from_numpy(buf.copy()).cuda()
    d_off = torch.from_numpy(np.concatenate([[0], np.flatnonzero(buf == 10) + 1]).astype(np.int64)).cuda()
    d_ps2, d_ops = torch.full((65,), FILL, dtype=torch.int64, device="cuda"), torch.full((65,), FILL, dtype=torch.int64, device="cuda")
    trace, ntr = np.full(16, -77, np.int64), C.c_int64(-77)
    torch.cuda.synchronize()                                  # (torch's fills run on its own stream)
    keep = (ci, hi, d_text, d_off, d_ps2, d_ops, trace, ntr, r, s, ps)
    ops = {
        "rfx_dev_dyn_pack": lambda co: L.rfx_dev_dyn_pack(ctx, C.byref(hi), C.byref(co)),
        "rfx_dev_dyn_binarize": lambda co: L.rfx_dev_dyn_binarize(ctx, d_text.data_ptr(), d_off.data_ptr(), r.n, 1, C.byref(co)),
        "rfx_dev_dyn_sort": lambda co: L.rfx_dev_dyn_sort(ctx, C.byref(ci), P, C.byref(co), d_ps2.data_ptr()),
        "rfx_dev_dyn_random_reflection": lambda co: L.rfx_dev_dyn_random_reflection(ctx, C.byref(ci), ps.data_ptr(), P, C.byref(co)),
        "rfx_dev_dyn_extend_pass": lambda co: L.rfx_dev_dyn_extend_pass(ctx, C.byref(ci), ps.data_ptr(), P, 1, 5, 2, C.byref(co), d_ops.data_ptr()),
        "rfx_dev_dyn_run": lambda co: L.rfx_dev_dyn_run(ctx, C.byref(ci), P, 1, 1, 5, 6, C.byref(co), trace.ctypes.data, 16, C.addressof(ntr)),
    }
    side = lambda: bool((d_ps2 == d_ps2[0]).all()) and bool((d_ops == d_ops[0]).all()) and int(d_ps2[0]) == int(d_ops[0]) != 0
    return ops, side, keep


def test_a_short_output_is_refused_with_the_needs_and_nothing_written(rfx):
    """cap_n = need - 1, then cap_words = need - 1: RFX_E_CAP with n / need_words set and every output tensor (0xA5) as it was; with
    exactly the needs the same call succeeds"""
    r, s, ps = small_sorted_set(rfx)
    ops, side, keep = operators(rfx, r, s, ps)
    for name, call in ops.items():
        big = poisoned(r.n, s.words + 8)
        co = big._c()
        assert call(co) == OK, name
        need_n, need_w = int(co.n), int(co.need_words)
        assert 0 < need_n <= r.n and 0 < need_w <= s.words, (name, need_n, need_w)
        exact = poisoned(need_n, need_w)
        assert call(exact._c()) == OK and not untouched(exact), name
        for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
            d = poisoned(cap_n, cap_w)
            co = d._c()
            co.n = co.need_words = -77
            assert call(co) == E_CAP, (name, cap_n, cap_w)
            assert (int(co.n), int(co.need_words)) == (need_n, need_w), name
            assert untouched(d), (name, cap_n, cap_w)


def test_a_key_of_125_bases_is_refused_by_pack_binarize_and_every_operator(rfx):
    """RFX_E_LIMIT with nothing written: from the host form and the text (a 125-base key among shorter ones), and from every operator
    on a packed set whose key_len holds 125"""
    import torch
    from reflexiv_amd.api import DynRecords
    rng = np.random.default_rng(82)
    r, s, ps = small_sorted_set(rfx)
    rows = r.rows()
    rows.insert(5, ("".join(NUC[b] for b in rng.integers(0, 4, 125)), "1|-3|-4", "ACGT"))
    long = DynRecords.from_rows(rows)
    bad = rfx.dyn_pack(r)
    bad.key_len[7] = 125
    torch.cuda.synchronize()
    for src, which in ((long, ("rfx_dev_dyn_pack", "rfx_dev_dyn_binarize")),
                       (r, ("rfx_dev_dyn_sort", "rfx_dev_dyn_random_reflection", "rfx_dev_dyn_extend_pass", "rfx_dev_dyn_run"))):
        ops, side, keep = operators(rfx, src, bad, ps)
        for name in which:
            d = poisoned(long.n, s.words + 64)
            co = d._c()
            co.n = co.need_words = -77
            assert ops[name](co) == E_LIMIT, name
            assert untouched(d) and (int(co.n), int(co.need_words)) == (-77, -77) and side(), name
            assert keep[7].value == -77 and (keep[6] == -77).all(), name
    ln = C.c_int64(-77)
    d_text = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert rfx.L.rfx_dev_dyn_to_text(rfx.ctx, C.byref(bad._c()), d_text.data_ptr(), 4096, C.addressof(ln)) == E_LIMIT
    assert ln.value == -77 and bool((d_text == FILL).all())


@pytest.mark.parametrize("P", [0, 64])
def test_a_partition_count_out_of_range_is_refused(rfx, P):
    r, s, ps = small_sorted_set(rfx)
    ops, side, keep = operators(rfx, r, s, ps, P)
    for name in ("rfx_dev_dyn_sort", "rfx_dev_dyn_random_reflection", "rfx_dev_dyn_extend_pass", "rfx_dev_dyn_run"):
        d = poisoned(r.n, s.words)
        assert ops[name](d._c()) == E_ARG, name
        assert untouched(d) and side(), name
    out, ln = np.full(64, FILL, np.uint8), C.c_int64(-77)
    off = np.array([0, 8], np.int64)
    st = rfx.L.rfx_dyn_run_text(rfx.ctx, b"ACGT,1|2", off.ctypes.data, 1, 0, P, 1, 4, 1, 0, out.ctypes.data, 64, C.addressof(ln), None, 0, None)
    assert st == E_ARG and ln.value == -77 and (out == FILL).all()
    # a bad form, stage and start marker
    d = poisoned(r.n, s.words)
    ci = s._c()
    assert rfx.L.rfx_dev_dyn_extend_pass(rfx.ctx, C.byref(ci), ps.data_ptr(), 3, 2, 5, 2, C.byref(d._c()), None) == E_ARG
    assert rfx.L.rfx_dev_dyn_extend_pass(rfx.ctx, C.byref(ci), ps.data_ptr(), 3, 1, 5, 3, C.byref(d._c()), None) == E_ARG
    assert rfx.L.rfx_dev_dyn_binarize(rfx.ctx, ps.data_ptr(), ps.data_ptr(), 1, 2, C.byref(d._c())) == E_ARG
    assert rfx.L.rfx_dev_dyn_sort(rfx.ctx, None, 3, C.byref(d._c()), ps.data_ptr()) == E_ARG
    assert untouched(d)


def test_text_buffers_one_byte_short(rfx):
    """rfx_dev_dyn_to_text and rfx_dyn_run_text with cap = length - 1: RFX_E_CAP, the needed length, nothing at or past cap written"""
    import torch
    r, s, ps = small_sorted_set(rfx)
    text = "".join(",".join(f) + "\n" for f in r.rows()).encode()
    full, need = rfx.dyn_to_text_dev(s)
    assert bytes(full[:need].cpu().numpy()) == text
    d_text = torch.full((need + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ln = C.c_int64(0)
    assert rfx.L.rfx_dev_dyn_to_text(rfx.ctx, C.byref(s._c()), d_text.data_ptr(), need - 1, C.addressof(ln)) == E_CAP
    assert ln.value == need and bool((d_text[need - 1:] == FILL).all()) and bytes(d_text[:need - 1].cpu().numpy()) == text[:need - 1]
    assert rfx.L.rfx_dev_dyn_to_text(rfx.ctx, C.byref(s._c()), d_text.data_ptr(), need, C.addressof(ln)) == OK
    want, tr = rfx.dyn_run_text(text, 1, 3, start_iteration=5, end_iteration=6)
    off = np.concatenate([[0], np.flatnonzero(np.frombuffer(text, np.uint8) == 10) + 1]).astype(np.int64)
    out, trace, ntr = np.full(len(want) + 16, FILL, np.uint8), np.zeros(8, np.int64), C.c_int64(0)
    st = rfx.L.rfx_dyn_run_text(rfx.ctx, text, off.ctypes.data, len(off) - 1, 1, 3, 0, 0, 5, 6, out.ctypes.data, len(want) - 1, C.addressof(ln),
                                trace.ctypes.data, 8, C.addressof(ntr))
    assert st == E_CAP and ln.value == len(want) and (out[len(want) - 1:] == FILL).all() and out[:len(want) - 1].tobytes() == want[:-1]
    assert [int(x) for x in trace[:ntr.value]] == tr


def test_an_empty_set_through_every_entry_point(rfx):
    import torch
    from reflexiv_amd.api import DynRecords
    r = DynRecords.from_rows([])
    pk = rfx.dyn_pack(r)
    assert pk.n == 0 and pk.words == 0 and rfx.dyn_unpack(pk).n == 0
    s, ps = rfx.dyn_sort_dev(pk, 4)
    assert s.n == 0 and ps.cpu().tolist() == [0] * 5
    assert rfx.dyn_random_reflection_dev(s, ps).n == 0
    g, ops = rfx.dyn_extend_pass_dev(s, ps, 1, 5, 2)
    assert g.n == 0 and ops.cpu().tolist() == [0] * 5
    out, tr = rfx.dyn_run_dev(pk, 4, True, 4, 5, 6)
    assert out.n == 0 and tr == [0] * 6
    torch.cuda.synchronize()
    b = rfx.dyn_binarize_dev(torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), 0)
    assert b.n == 0
    assert rfx.dyn_to_text_dev(out)[1] == 0
    assert rfx.dyn_run_text(b"", 0, 4, True, 4) == (b"", [0] * 4)
    assert rfx.dyn_run_text(b"\n\r\n", 1, 2, start_iteration=5, end_iteration=5) == (b"", [0])
    for t in (pk, s, g, out, b):
        assert int(t.ext_off[0]) == 0


# ---- 6. poisoned allocations ---------------------------------------------------------------------------------------------------------------
def test_packed_passes_hold_with_every_allocation_poisoned():
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
