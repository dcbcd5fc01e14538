"""The k-mer sorting stage (Count_<k>_sorted) on packed record sets in HBM (rfx_dev_ksort_*, rfx_ksort_text):
every operator against its stage of the rows the reference's own classes made (tests/golden/ksort_vectors.npz), unpacked field by
field and as raw words against the numpy packer (zero padding bits, zero unused key words); the resident chain and the host form
against the final text; row counts around the block size, runs placed on block edges and the 600-row run against the string model
(tests/ksort_model.py, which test_ksort_model.py pins to the same vectors); the argument, capacity and text-buffer contracts; the
hand-over to rfx_dev_dyn_binarize form 0 and rfx_dev_dyn_sort; and all of it again with every allocation poisoned."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ksort_model as K
from tests.test_gpu_dynamic_edges import same_records
from tests.test_gpu_dynamic_packed import raw_equals, poisoned, untouched, FILL, OK, E_ARG, E_CAP

pytestmark = pytest.mark.gpu

VEC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ksort_vectors.npz")
COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 16, 18, 29999, 30000)


def case_names():
    return [str(x) for x in np.load(VEC)["names"]]


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


@pytest.fixture(scope="module")
def vec():
    """every case, loaded once: name -> (params dict, rows, {stage: records}, text)"""
    z = np.load(VEC)
    return {n: K.load_case(z, n) for n in case_names()}


def cparams(rfx, p):
    return rfx.ksort_params(p["k"], max_k=p["max_k"], min_error_cov=p["min_error_cov"], max_cov=p["max_cov"], bubble=p["bubble"],
                            min_repeat_fold=p["min_repeat_fold"])


def host(recs):
    from reflexiv_amd.api import DynRecords
    return DynRecords.from_text([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs], [r[4] for r in recs])


def upload(rows):
    """rows (each with its line end) -> (d_text, d_row_off) in HBM"""
    import torch
    buf = np.frombuffer("".join(rows).encode(), np.uint8)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    d = (torch.from_numpy(buf.copy() if len(buf) else np.zeros(1, np.uint8)).cuda(), torch.from_numpy(off).cuda())
    torch.cuda.synchronize()
    return d


def equals(rfx, pk, recs, tag):
    """the packed set in HBM is the record list: unpacked field by field, and word for word the numpy packer's"""
    want = host(recs)
    same_records(rfx.dyn_unpack(pk), want, tag)
    raw_equals(pk, want, tag)


def text_of(rfx, pk, k):
    d_text, ln, d_off, rows = rfx.ksort_to_text_dev(pk, k)
    text = bytes(d_text[:ln].cpu().numpy())
    off = d_off[:rows + 1].cpu().numpy()
    assert rows == text.count(b"\n") and off[0] == 0 and off[-1] == ln
    assert all(text[a:b].endswith(b"\n") and text[a:b].count(b"\n") == 1 for a, b in zip(off[:-1], off[1:]))
    return text.decode()


def chain(rfx, rows, p):
    """the operators one by one on the device -> {stage: packed set}"""
    cp = cparams(rfx, p)
    st = {"s4": rfx.ksort_binarize(*upload(rows), cp)}
    cur = st["s4"]
    if p["bubble"]:
        st["s5_sort"], _ = rfx.dyn_sort_dev(cur, 1)
        st["s5_fold"] = rfx.ksort_fork_filter(st["s5_sort"], False, cp)
        st["s6"] = rfx.ksort_reflect(st["s5_fold"])
        st["s7_sort"], _ = rfx.dyn_sort_dev(st["s6"], 1)
        st["s7_fold"] = cur = rfx.ksort_fork_filter(st["s7_sort"], True, cp)
    st["s8"] = rfx.ksort_full_kmers(cur)
    return st


# ---- 1. every operator against the reference's classes -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", case_names())
def test_every_operator_equals_its_stage_of_the_reference(rfx, vec, case):
    """each operator is fed the reference's previous output (packed by rfx_dev_dyn_pack); bubble = 0 (k33_bubble0) has steps 4 and 8
    only; k41_longrun holds a run of 1200 equal keys in the forward fold"""
    p, rows, st, text = vec[case]
    cp = cparams(rfx, p)
    equals(rfx, rfx.ksort_binarize(*upload(rows), cp), st["s4"], (case, "s4"))
    last = "s4"
    if p["bubble"]:
        for src, dst, fn in (("s4", "s5_sort", lambda d: rfx.dyn_sort_dev(d, 1)[0]),
                             ("s5_sort", "s5_fold", lambda d: rfx.ksort_fork_filter(d, False, cp)),
                             ("s5_fold", "s6", rfx.ksort_reflect),
                             ("s6", "s7_sort", lambda d: rfx.dyn_sort_dev(d, 3)[0]),
                             ("s7_sort", "s7_fold", lambda d: rfx.ksort_fork_filter(d, True, cp))):
            pk = rfx.dyn_pack(host(st[src]))
            g = fn(pk)
            equals(rfx, g, st[dst], (case, dst))
            assert g.n <= pk.n and g.words <= pk.words, (case, dst, "capacity bound")
        last = "s7_fold"
    full = rfx.ksort_full_kmers(rfx.dyn_pack(host(st[last])))
    equals(rfx, full, st["s8"], (case, "s8"))
    assert full.words == 0
    assert text_of(rfx, rfx.dyn_pack(host(st["s8"])), p["k"]) == text, (case, "text")


@pytest.mark.parametrize("case", case_names())
def test_the_resident_chain_and_the_host_form_equal_the_final_text(rfx, vec, case):
    p, rows, st, text = vec[case]
    cp = cparams(rfx, p)
    out = rfx.ksort_run(*upload(rows), cp)
    equals(rfx, out, st["s8"], (case, "run"))
    assert text_of(rfx, out, p["k"]) == text
    assert rfx.ksort_text("".join(rows).encode(), cp).decode() == text
    assert rfx.last_call_ms > 0


# ---- 2. row counts around the block size, against the model --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 127, 128, 129, 255, 256, 257, 3000])
def test_row_counts_around_the_block_size(rfx, vec, n):
    """the first n rows of k41_longrun (971 rows, tiled for 3000 -- duplicates lengthen the runs): every stage of the chain composed
    from the operators, the resident chain and its text against the string model"""
    p, rows, _, _ = vec["k41_longrun"]
    rows = (rows * 4)[:n]
    want = K.run_stages(rows, p)
    got = chain(rfx, rows, p)
    for s in K.STAGES:
        equals(rfx, got[s], want[s], (n, s))
    out = rfx.ksort_run(*upload(rows), cparams(rfx, p))
    equals(rfx, out, want["s8"], (n, "run"))
    assert text_of(rfx, out, p["k"]) == K.to_text(want["s8"], p["k"])


# ---- 3. runs on block edges ----------------------------------------------------------------------------------------------------------
def sorted_runs(rng, k1, lengths, M, marker):
    """a sorted set: run j has lengths[j] records of one random key of k1 bases"""
    keys = set()
    while len(keys) < len(lengths):
        keys.add("".join("ACGT"[b] for b in rng.integers(0, 4, k1)))
    keys = [r[0] for r in K.sort_records([(s, "A", 1, 1, 1) for s in keys])]
    return [(key, "ACGT"[int(rng.integers(0, 4))], marker, int(rng.choice(COUNTS)), int(rng.choice((-1, M))))
            for key, ln in zip(keys, lengths) for _ in range(ln)]


@pytest.mark.parametrize("reflected", [False, True])
@pytest.mark.parametrize("k1", [30, 64, 123])
def test_runs_that_end_and_start_on_block_edges(rfx, reflected, k1):
    """blocks of 256 threads: single records pad the set so that a run of 7 ends on thread 255 of block 0, a run of 5 starts on
    thread 0 of block 1, a run of 450 covers all of block 2 from inside block 1 into block 3, and a run of 4 ends on the set's last record"""
    p = K.default_params(k1 + 1, max_k=97)
    lengths = [1] * 249 + [7] + [5] + [1] * 100 + [450] + [1] * 20 + [4]
    recs = sorted_runs(np.random.default_rng(90 + k1), k1, lengths, p["max_k"] + 3, 2 if reflected else 1)
    starts = np.cumsum([0] + lengths)
    assert starts[250] == 256 and starts[249] + 7 == 256 and starts[351] < 512 and starts[352] > 768
    want = K.fork_filter(recs, reflected, p)
    assert len(want) == len(lengths)
    g = rfx.ksort_fork_filter(rfx.dyn_pack(host(recs)), reflected, cparams(rfx, p))
    equals(rfx, g, want, ("edges", reflected, k1))


def test_the_600_row_run(rfx, vec):
    """k41_longrun: 600 rows of one k-mer -> runs of 600 in the forward fold (the k-mer's and its reverse complement's), crossing two
    block edges"""
    p, rows, st, text = vec["k41_longrun"]
    from collections import Counter
    assert max(Counter(r[0] for r in st["s5_sort"]).values()) >= 600
    got = chain(rfx, rows, p)
    for s in K.STAGES:
        equals(rfx, got[s], st[s], ("longrun", s))


# ---- 4. contracts --------------------------------------------------------------------------------------------------------------------
def thunks(rfx, vec):
    """every entry point with a packed output, as thunks (params, output struct) -> status, on the stages of k33_m33"""
    p, rows, st, _ = vec["k33_m33"]
    L, ctx = rfx.L, rfx.ctx
    d_text, d_off = upload(rows)
    s5, s5f, s7, s7f = (rfx.dyn_pack(host(st[s])) for s in ("s5_sort", "s5_fold", "s7_sort", "s7_fold"))
    ci = {n: d._c() for n, d in (("s5", s5), ("s5f", s5f), ("s7", s7), ("s7f", s7f))}
    keep = (d_text, d_off, s5, s5f, s7, s7f, ci)
    ops = {
        "binarize": lambda cp, co: L.rfx_dev_ksort_binarize(ctx, d_text.data_ptr(), d_off.data_ptr(), len(rows), C.byref(cp), C.byref(co)),
        "fork_filter 0": lambda cp, co: L.rfx_dev_ksort_fork_filter(ctx, 0, C.byref(ci["s5"]), C.byref(cp), C.byref(co)),
        "fork_filter 1": lambda cp, co: L.rfx_dev_ksort_fork_filter(ctx, 1, C.byref(ci["s7"]), C.byref(cp), C.byref(co)),
        "reflect": lambda cp, co: L.rfx_dev_ksort_reflect(ctx, C.byref(ci["s5f"]), C.byref(co)),
        "full_kmers": lambda cp, co: L.rfx_dev_ksort_full_kmers(ctx, C.byref(ci["s7f"]), C.byref(co)),
        "run": lambda cp, co: L.rfx_dev_ksort_run(ctx, d_text.data_ptr(), d_off.data_ptr(), len(rows), C.byref(cp), C.byref(co)),
    }
    return p, rows, ops, keep


@pytest.mark.parametrize("k", [32, 63, 94, 7, 125])
def test_a_refused_k_returns_the_code_and_writes_nothing(rfx, vec, k):
    p, rows, ops, keep = thunks(rfx, vec)
    cp = cparams(rfx, dict(p, k=k))
    for name in ("binarize", "fork_filter 0", "fork_filter 1", "run"):
        d = poisoned(2 * len(rows), 2 * len(rows))
        co = d._c()
        co.n = co.need_words = -77
        assert ops[name](cp, co) == E_ARG, (name, k)
        assert untouched(d) and (int(co.n), int(co.need_words)) == (-77, -77), (name, k)
    out, ln = np.full(64, FILL, np.uint8), C.c_int64(-77)
    off = np.array([0, 10], np.int64)
    assert rfx.L.rfx_ksort_text(rfx.ctx, b"ACGTACGT,3", off.ctypes.data, 1, C.byref(cp), out.ctypes.data, 64, C.addressof(ln)) == E_ARG
    assert ln.value == -77 and (out == FILL).all()


BAD_ROWS = {"no comma": "ACGTACGTAC 5\n", "empty count": "ACGTACGTAC,\n", "letters": "ACGTACGTAC,1x\n", "sign": "ACGTACGTAC,-3\n",
            "plus": "ACGTACGTAC,+3\n", "only a bracket": "ACGTACGTAC,)\n", "two commas": "ACGTACGTAC,3,4\n", "blank": "\n",
            "bad count on a row of another length": "ACGT,x\n"}


@pytest.mark.parametrize("form", sorted(BAD_ROWS))
def test_a_malformed_row_returns_e_arg_and_writes_nothing(rfx, form):
    good = ["ACGTACGTAA,3\n", "(CCGTACGTAA,4)\n", "TTGTACGTAA,0000000005\n"]
    cp = rfx.ksort_params(10)
    assert K.run_text(good, K.default_params(10)) == rfx.ksort_text("".join(good).encode(), cp).decode()
    rows = good[:2] + [BAD_ROWS[form]] + good[2:]
    with pytest.raises(K.BadRow):
        K.binarize(rows, K.default_params(10))
    d_text, d_off = upload(rows)
    for fn in (rfx.L.rfx_dev_ksort_binarize, rfx.L.rfx_dev_ksort_run):
        d = poisoned(8, 8)
        co = d._c()
        co.n = co.need_words = -77
        assert fn(rfx.ctx, d_text.data_ptr(), d_off.data_ptr(), len(rows), C.byref(cp), C.byref(co)) == E_ARG, form
        assert untouched(d) and (int(co.n), int(co.need_words)) == (-77, -77), form


def test_bad_parameters_null_pointers_and_mixed_key_lengths(rfx, vec):
    import torch
    p, rows, ops, keep = thunks(rfx, vec)
    d = poisoned(2 * len(rows), 2 * len(rows))
    for bad in (dict(min_error_cov=0), dict(min_error_cov=-1), dict(min_repeat_fold=0.99), dict(min_repeat_fold=float("nan")), dict(max_k=0)):
        cp = cparams(rfx, dict(p, **bad))
        for name in ("binarize", "fork_filter 0", "fork_filter 1", "run"):
            assert ops[name](cp, d._c()) == E_ARG, (name, bad)
    cp = cparams(rfx, p)
    L, ctx, ci = rfx.L, rfx.ctx, keep[6]
    assert L.rfx_dev_ksort_binarize(ctx, None, keep[1].data_ptr(), len(rows), C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_ksort_binarize(ctx, keep[0].data_ptr(), keep[1].data_ptr(), len(rows), None, C.byref(d._c())) == E_ARG
    assert L.rfx_dev_ksort_run(ctx, keep[0].data_ptr(), keep[1].data_ptr(), len(rows), C.byref(cp), None) == E_ARG
    assert L.rfx_dev_ksort_fork_filter(ctx, 0, None, C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_ksort_fork_filter(ctx, 2, C.byref(ci["s5"]), C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_ksort_reflect(ctx, C.byref(ci["s5f"]), None) == E_ARG
    assert L.rfx_dev_ksort_full_kmers(ctx, None, C.byref(d._c())) == E_ARG
    no_key = d._c()
    no_key.key = None
    assert L.rfx_dev_ksort_reflect(ctx, C.byref(ci["s5f"]), C.byref(no_key)) == E_ARG
    # keys of two lengths; an extension that is not one base
    mixed = rfx.dyn_pack(host([("ACGTACGTA", "C", 1, 3, 3), ("ACGTACGTAC", "C", 1, 3, 3)]))
    long_ext = rfx.dyn_pack(host([("ACGTACGTA", "CC", 1, 3, 3), ("ACGTACGTC", "C", 1, 3, 3)]))
    cm, cl = mixed._c(), long_ext._c()
    assert L.rfx_dev_ksort_fork_filter(ctx, 0, C.byref(cm), C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_ksort_fork_filter(ctx, 1, C.byref(cm), C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_ksort_reflect(ctx, C.byref(cm), C.byref(d._c())) == E_ARG
    for fn in (L.rfx_dev_ksort_reflect, L.rfx_dev_ksort_full_kmers):
        assert fn(ctx, C.byref(cl), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_ksort_fork_filter(ctx, 0, C.byref(cl), C.byref(cp), C.byref(d._c())) == E_ARG
    ln, nr = C.c_int64(-77), C.c_int64(-77)
    d_text = torch.full((64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert L.rfx_dev_ksort_to_text(ctx, None, 33, d_text.data_ptr(), 64, C.addressof(ln), None, C.addressof(nr)) == E_ARG
    assert L.rfx_dev_ksort_to_text(ctx, C.byref(ci["s7f"]), 33, d_text.data_ptr(), 64, None, None, C.addressof(nr)) == E_ARG
    assert untouched(d) and (ln.value, nr.value) == (-77, -77) and bool((d_text == FILL).all())


def test_every_capacity_one_short(rfx, vec):
    """cap_n = need - 1, then cap_words = need - 1: RFX_E_CAP with n / need_words set and every output tensor (0xA5) as it was; with
    exactly the needs the same call succeeds.  full_kmers and run need no extension words: cap_words = 0 is enough"""
    p, rows, ops, keep = thunks(rfx, vec)
    cp = cparams(rfx, p)
    for name, call in ops.items():
        big = poisoned(2 * len(rows), 2 * len(rows))
        co = big._c()
        assert call(cp, co) == OK, name
        need_n, need_w = int(co.n), int(co.need_words)
        assert 0 < need_n <= 2 * len(rows) and need_w == (0 if name in ("full_kmers", "run") else need_n), (name, need_n, need_w)
        exact = poisoned(need_n, need_w)
        assert call(cp, exact._c()) == OK and not untouched(exact), name
        for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
            if cap_w < 0:
                continue
            d = poisoned(cap_n, cap_w)
            co = d._c()
            co.n = co.need_words = -77
            assert call(cp, co) == E_CAP, (name, cap_n, cap_w)
            assert (int(co.n), int(co.need_words)) == (need_n, need_w), name
            assert untouched(d), (name, cap_n, cap_w)


def test_text_buffers_one_byte_short(rfx, vec):
    """rfx_dev_ksort_to_text and rfx_ksort_text with cap = length - 1: RFX_E_CAP, the needed length, nothing at or past cap written"""
    import torch
    p, rows, st, text = vec["k33_m33"]
    text = text.encode()
    need = len(text)
    pk = rfx.dyn_pack(host(st["s8"]))
    d_text = torch.full((need + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ln, nr = C.c_int64(0), C.c_int64(0)
    ci = pk._c()
    assert rfx.L.rfx_dev_ksort_to_text(rfx.ctx, C.byref(ci), p["k"], d_text.data_ptr(), need - 1, C.addressof(ln), None, C.addressof(nr)) == E_CAP
    assert (ln.value, nr.value) == (need, pk.n) and bool((d_text[need - 1:] == FILL).all()) and bytes(d_text[:need - 1].cpu().numpy()) == text[:-1]
    assert rfx.L.rfx_dev_ksort_to_text(rfx.ctx, C.byref(ci), p["k"], d_text.data_ptr(), need, C.addressof(ln), None, C.addressof(nr)) == OK
    assert bytes(d_text[:need].cpu().numpy()) == text and bool((d_text[need:] == FILL).all())
    src = "".join(rows).encode()
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    out = np.full(need + 16, FILL, np.uint8)
    cp = cparams(rfx, p)
    assert rfx.L.rfx_ksort_text(rfx.ctx, src, off.ctypes.data, len(rows), C.byref(cp), out.ctypes.data, need - 1, C.addressof(ln)) == E_CAP
    assert ln.value == need and (out[need - 1:] == FILL).all() and out[:need - 1].tobytes() == text[:-1]
    assert rfx.L.rfx_ksort_text(rfx.ctx, src, off.ctypes.data, len(rows), C.byref(cp), out.ctypes.data, need, C.addressof(ln)) == OK
    assert out[:need].tobytes() == text


def test_to_text_drops_the_records_of_another_length(rfx):
    recs = [("ACGTACGTAC", "", 1, -1, 98), ("ACGTACGTA", "", 1, 5, 5), ("CCGTACGTAC", "", 1, 30000, -1), ("ACGTACGTACG", "", 1, 1, 1)]
    assert text_of(rfx, rfx.dyn_pack(host(recs)), 10) == K.to_text(recs, 10) == "ACGTACGTAC,1|-1|98\nCCGTACGTAC,1|30000|-1\n"


@pytest.mark.parametrize("shift", [1, 3, 8])
def test_to_text_into_a_buffer_at_any_alignment(rfx, vec, shift):
    """the fill stores whole 8-byte chunks where the destination is aligned and single bytes where it is not"""
    import torch
    p, rows, st, text = vec["k23_m23"]
    buf = torch.full((len(text) + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d_text, ln, _, n = rfx.ksort_to_text_dev(rfx.dyn_pack(host(st["s8"])), p["k"], buf[shift:shift + len(text)], want_offsets=False)
    assert ln == len(text) and bytes(buf[shift:shift + ln].cpu().numpy()).decode() == text
    assert bool((buf[:shift] == FILL).all()) and bool((buf[shift + ln:] == FILL).all())


def test_an_empty_input_through_every_entry_point(rfx):
    cp = rfx.ksort_params(31)
    b = rfx.ksort_binarize(*upload([]), cp)
    assert b.n == 0
    s, _ = rfx.dyn_sort_dev(b, 1)
    outs = [b, rfx.ksort_fork_filter(s, False, cp), rfx.ksort_fork_filter(s, True, cp), rfx.ksort_reflect(s), rfx.ksort_full_kmers(s),
            rfx.ksort_run(*upload([]), cp), rfx.ksort_run(*upload(["ACGT,5\n"]), cp)]          # (a row of another length: dropped)
    for t in outs:
        assert t.n == 0 and int(t.ext_off[0]) == 0
    d_text, ln, d_off, rows = rfx.ksort_to_text_dev(b, 31)
    assert (ln, rows) == (0, 0) and int(d_off[0]) == 0
    assert rfx.ksort_text(b"", cp) == b""


# ---- 5. the hand-over to the dynamic-k passes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k31_m31", "k64_m97", "k95_m95"])
def test_the_text_and_its_row_offsets_go_straight_to_the_dynamic_k_binarizer(rfx, vec, case):
    """d_text and d_row_off of rfx_dev_ksort_to_text -> rfx_dev_dyn_binarize form 0: key = the k-mer without its last base, extension =
    that base, orientation 1, the attributes read back; rfx_dev_dyn_sort accepts the result"""
    p, rows, st, text = vec[case]
    out = rfx.ksort_run(*upload(rows), cparams(rfx, p))
    d_text, ln, d_off, n = rfx.ksort_to_text_dev(out, p["k"])
    pk = rfx.dyn_binarize_dev(d_text[:ln], d_off[:n + 1], 0)
    want = K.handover(text)
    assert len(want) == n == out.n
    equals(rfx, pk, want, (case, "hand-over"))
    s, ps = rfx.dyn_sort_dev(pk, 4)
    equals(rfx, s, K.sort_records(want), (case, "hand-over, sorted"))
    assert ps.cpu().tolist()[0] == 0 and ps.cpu().tolist()[-1] == n


def test_reflexiv_host_sort_writes_the_case_text(vec, tmp_path):
    """`reflexiv_host sort -kmerc COUNTS -kmer K -klist ... -outfile O` -> O/Count_K_sorted/part-00000.csv; max_k = the last k of
    -klist; -error reaches the folds"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reflexiv_amd", "reflexiv_host")
    for case, extra in (("k33_m97", ["-klist", "27,33,97"]), ("k31_m31", ["-klist", "31"]), ("k23_m97", ["-klist", "23,97"])):
        p, rows, st, text = vec[case]
        src, out = tmp_path / (case + ".csv"), tmp_path / case
        src.write_text("".join(rows))
        r = subprocess.run([exe, "sort", "-kmerc", str(src), "-kmer", str(p["k"]), "-outfile", str(out)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert (out / f"Count_{p['k']}_sorted" / "part-00000.csv").read_text() == text, case
        assert (out / f"Count_{p['k']}_sorted" / "_SUCCESS").exists()


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
