"""The capacity contract of every entry point that writes into a caller's buffer of `cap` entries (DESIGN.md "Capacity
contract"): a short `cap` is the normal first call of rfx_assemble_reads and `counter --resident`, which start small and
grow on RFX_E_CAP.

Guard-band harness: the expected survivors come from the CPU oracle (need = their number); every output array is allocated
with need + G entries and filled with the byte 0xA5 before every call (never a valid output: a k <= 31 key has bits 62..63
clear, the last word of a W-word key holds at most 62 bits, counts are non-negative, and the leaf tables' EMPTY is all ones);
only the `cap` ARGUMENT shrinks, so a kernel that ignored it would still write inside memory the test owns.  For
cap < need: RFX_E_CAP, the reported need equals the oracle's, nothing at or past `cap` was written, and the next call with
cap = need gives exactly the oracle's answer and leaves [need, need + G) alone; cap = need and need + 1 succeed likewise.
Bit-exact (integer work)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_ragged_w import host_bin, upload, write_fq

pytestmark = pytest.mark.gpu

G = 4096                    # guard entries behind every output array
FILL = 0xA5
OK, E_ARG, E_CAP = 0, -1, -2


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


# ------------------------------------------------------------------ inputs and their oracle answers (computed once)

class Base:
    """one read set on the host and on the device, and the oracle's k-mers / survivors of it by (k, min_cov)"""

    def __init__(self, rfx, torch, bases, off):
        self.bases, self.off = np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(off, np.int64)
        self.dw, self.dl, self.n, self.wpr, self.L = upload(rfx, torch, self.bases, self.off)
        self._km, self._want = {}, {}

    def km(self, k):
        if k not in self._km:
            self._km[k] = O.extract_canon(self.bases, self.off, k) if k <= 31 else O.extract_canon_w(self.bases, self.off, k)
        return self._km[k]

    def want(self, k, min_cov):
        if (k, min_cov) not in self._want:
            wk, wc, wd = O.count_filter(self.km(k), min_cov) if k <= 31 else O.count_filter_w(self.km(k), k, min_cov)
            print(f"k = {k}: {len(self.km(k))} instances, {len(wk)} survivors at min_cov {min_cov}, {wd} distinct")
            self._want[(k, min_cov)] = (wk, wc, wd)
        return self._want[(k, min_cov)]


_bases = {}


def base_for(rfx, torch, k):
    """k <= 31: O.synth_genome(5, 20000), 6000 reads of 100 bases; k > 31: the same genome, 3000 reads of k + 40 bases"""
    L, n = (100, 6000) if k <= 31 else (k + 40, 3000)
    if L not in _bases:
        g = O.synth_genome(5, 20_000)
        _bases[L] = Base(rfx, torch, *O.synth_reads(5, g, 20_000, 0, n, L))
    return _bases[L]


def kernel_constants():
    """the leaf kernels' LDS survivor buffers, read off rfx_kmer.hip: (OBT of k-mer / pair leaves, OBT of record leaves,
    WOBUF of the two- and W-word leaves)"""
    import reflexiv_amd
    src = open(os.path.join(os.path.dirname(reflexiv_amd.__file__), "csrc", "rfx_kmer.hip")).read()
    c = {}
    for name in ("LT", "LOBUF", "LOBUF1", "WSTAGE", "WOBUF"):
        found = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert found, f"rfx_kmer.hip no longer has `constexpr int {name} = <number>;`: update kernel_constants() to the leaf kernels' buffers"
        c[name] = int(found.group(1))
    lstage = c["WSTAGE"] * (c["LT"] // 64)
    return c["LOBUF"], c["LOBUF1"] + (lstage * 8) // 12, c["WOBUF"]


# ------------------------------------------------------------------ the harness

def untouched(torch, t, start=0):
    """every byte of t[start:] is still the fill"""
    return bool((t[start:].contiguous().view(torch.uint8) == FILL).all())


def first_touched(torch, t, start):
    """(the first entries of t[start:] (rows of a 2-D t) that no longer hold the fill, how many there are)"""
    v = (t if t.dim() == 2 else t.view(-1, 1))[start:].contiguous().view(torch.uint8)
    bad = torch.nonzero((v != FILL).any(dim=1)).flatten()
    return [int(x) + start for x in bad[:8]], int(bad.numel())


def guard_band(torch, call, want_keys, want_counts, W, count_dtype, untouched_on_cap=False, where=""):
    """call(keys_ptr, counts_ptr, cap) -> (status, reported n).  Runs the cap ladder described in the module docstring.
    untouched_on_cap: the entry checks before it emits, so on RFX_E_CAP the WHOLE buffer must still hold the fill."""
    need = len(want_counts)
    assert need > 4
    dk = torch.empty((need + G) * W, dtype=torch.int64, device="cuda")
    dc = torch.empty(need + G, dtype=count_dtype, device="cuda")
    want_keys = np.ascontiguousarray(want_keys, np.uint64).reshape(need, W)

    def run(cap):
        dk.view(torch.uint8).fill_(FILL); dc.view(torch.uint8).fill_(FILL)
        torch.cuda.synchronize()
        st, n = call(dk.data_ptr(), dc.data_ptr(), cap)
        torch.cuda.synchronize()
        return st, n

    def check_ok(cap):
        st, n = run(cap)
        assert (st, n) == (OK, need), (where, cap, st, n, need)
        got_k = dk[:need * W].cpu().numpy().view(np.uint64).reshape(need, W)
        got_c = dc[:need].cpu().numpy()
        assert np.array_equal(got_k, want_keys) and np.array_equal(got_c, want_counts), (where, cap)
        assert untouched(torch, dk, need * W), (where, cap, "keys past need", first_touched(torch, dk.view(-1, W), need))
        assert untouched(torch, dc, need), (where, cap, "counts past need", first_touched(torch, dc, need))

    for cap in (0, 1, need // 2, need - 1):
        st, n = run(cap)
        assert st == E_CAP, (where, cap, st)
        assert n == need, (where, cap, n, need)
        lo = 0 if untouched_on_cap else cap
        assert untouched(torch, dk, lo * W), (where, cap, "keys at or past cap", first_touched(torch, dk.view(-1, W), lo))
        assert untouched(torch, dc, lo), (where, cap, "counts at or past cap", first_touched(torch, dc, lo))
        check_ok(need)
    check_ok(need)
    check_ok(need + 1)
    return need


def only_the_main_leaf_launch(t):
    """the leaf kernel was timed once: no leaf crossed the heavy threshold, so no slice launch and no k_reduce_partials ran,
    every survivor came out of the launch whose table passes stat_passes counts"""
    return t.get("leaf", (0, 0))[1] == 1


def wrapper_need(torch, call, need, W):
    """call(keys_ptr, counts_ptr, cap) goes through a Python wrapper: with cap = 7 it raises RfxError(RFX_E_CAP) whose .need is
    the capacity to retry with"""
    from reflexiv_amd import RfxError
    dk = torch.empty((need + G) * W, dtype=torch.int64, device="cuda"); dc = torch.empty(need + G, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(RfxError) as ei:
        call(dk.data_ptr(), dc.data_ptr(), 7)
    assert ei.value.status == E_CAP and ei.value.need == need, (ei.value.status, getattr(ei.value, "need", None), need)


def i64(v):
    return C.c_int64(int(v))


def ptr(v):
    return C.c_void_p(int(v))


BIG = 10_000_000


def call_count_reads(rfx, b, k, min_cov):
    def call(pk, pc, cap):
        n, d, inst = i64(0), i64(0), i64(0)
        st = rfx.L.rfx_dev_count_reads(rfx.ctx, ptr(b.dw.data_ptr()), i64(b.n), b.wpr, b.L, k, 0, 0, min_cov, BIG, O.TWIN_DS, None,
                                       i64(0), ptr(pk), ptr(pc), i64(cap), C.byref(n), C.byref(d), C.byref(inst))
        assert inst.value == len(b.km(k))
        return st, n.value
    return call


def call_count_reads_w(rfx, b, k, min_cov):
    def call(pk, pc, cap):
        n, d, inst = i64(0), i64(0), i64(0)
        st = rfx.L.rfx_dev_count_reads_w(rfx.ctx, ptr(b.dw.data_ptr()), i64(b.n), b.wpr, b.L, k, 0, 0, min_cov, BIG, ptr(pk), ptr(pc),
                                         i64(cap), C.byref(n), C.byref(d), C.byref(inst))
        assert inst.value == len(b.km(k))
        return st, n.value
    return call


# ------------------------------------------------------------------ rfx_dev_count_reads and its siblings, k <= 31

@pytest.mark.parametrize("k", [31, 21, 15])
def test_count_reads_buffered_flush(rfx, torch_mod, k):
    """min_cov 2 (k = 31, 21: record leaves, k = 15: k-mer leaves).  The branch: the first survivor of a workgroup's first
    pass always finds the LDS buffer empty, so with m > 0 survivors out of the leaf kernel ("leaf" launches > 0) the buffered
    flush has run; asserted below, with the leaf kernel timed once (no heavy slices: every survivor is the main launch's)."""
    torch = torch_mod
    b = base_for(rfx, torch, k)
    wk, wc, wd = b.want(k, 2)
    guard_band(torch, call_count_reads(rfx, b, k, 2), wk, wc, 1, torch.int32, where=f"count_reads k={k}")
    t = rfx.count_timing()
    assert only_the_main_leaf_launch(t) and t["stat_passes"][1] > 0 and len(wk) > 0, t


@pytest.mark.parametrize("k", [31, 21, 15])
def test_count_reads_wave_direct_write(rfx, torch_mod, k, monkeypatch):
    """min_cov 1 under RFX_LEVEL_BITS = "2,2" (16 leaves for the whole input): a table pass then yields more survivors than
    the LDS buffer holds (OBT = LOBUF for k-mer leaves, LOBUF1 + (LSTAGE * 8) / 12 for record leaves) and the wave writes
    straight to the output.  Proof that the branch ran: after the successful call m > stat_passes * OBT, so by pigeonhole at
    least one pass emitted more than the buffer takes; asserted below.  The leaf kernel was timed once, so no heavy slice ran
    and all m survivors belong to the passes counted."""
    torch = torch_mod
    monkeypatch.setenv("RFX_LEVEL_BITS", "2,2")
    b = base_for(rfx, torch, k)
    wk, wc, wd = b.want(k, 1)
    m = guard_band(torch, call_count_reads(rfx, b, k, 1), wk, wc, 1, torch.int32, where=f"count_reads k={k} bits 2,2")
    t = rfx.count_timing()
    ob_kmer, ob_rec, _ = kernel_constants()
    obt = ob_kmer if k == 15 else ob_rec
    print(f"k = {k}: m = {m}, table passes = {t['stat_passes'][1]}, OBT = {obt}")
    assert only_the_main_leaf_launch(t), t
    assert t["stat_passes"][1] > 0 and m > t["stat_passes"][1] * obt, (m, t, obt)


def test_count_reads_ragged(rfx, torch_mod):
    """rfx_dev_count_reads_ragged at k = 31: the base reads with a length array (every read 100 bases)"""
    torch = torch_mod
    k = 31
    b = base_for(rfx, torch, k)

    def call(pk, pc, cap):
        n, d, inst = i64(0), i64(0), i64(0)
        st = rfx.L.rfx_dev_count_reads_ragged(rfx.ctx, ptr(b.dw.data_ptr()), ptr(b.dl.data_ptr()), i64(b.n), b.wpr, b.L, k, 0, 0, 2, BIG,
                                              O.TWIN_DS, ptr(pk), ptr(pc), i64(cap), C.byref(n), C.byref(d), C.byref(inst))
        assert inst.value == len(b.km(k))
        return st, n.value
    wk, wc, wd = b.want(k, 2)
    guard_band(torch, call, wk, wc, 1, torch.int32, where="count_reads_ragged")
    assert rfx.count_timing().get("leaf", (0, 0))[1] > 0


@pytest.mark.parametrize("k,min_cov", [(31, 2), (15, 1)])
def test_count_kmers(rfx, torch_mod, k, min_cov):
    """rfx_dev_count_kmers: the oracle's k-mer instances as an explicit array (k-mer leaves, LOBUF survivors buffered)"""
    torch = torch_mod
    b = base_for(rfx, torch, k)
    km = b.km(k)
    dkm = torch.from_numpy(km.view(np.int64).copy()).cuda()

    def call(pk, pc, cap):
        n, d = i64(0), i64(0)
        st = rfx.L.rfx_dev_count_kmers(rfx.ctx, ptr(dkm.data_ptr()), i64(len(km)), min_cov, BIG, O.TWIN_DS, None, i64(0), ptr(pk), ptr(pc),
                                       i64(cap), C.byref(n), C.byref(d))
        return st, n.value
    wk, wc, wd = b.want(k, min_cov)
    guard_band(torch, call, wk, wc, 1, torch.int32, where=f"count_kmers k={k}")
    wrapper_need(torch, lambda pk, pc, cap: rfx.count_kmers_dev(dkm.data_ptr(), len(km), pk, pc, cap, min_cov), len(wk), 1)
    assert rfx.count_timing().get("leaf", (0, 0))[1] > 0


@pytest.mark.parametrize("k,min_cov,heavy", [(31, 2, "40,16,64"), (21, 1, "300,128,64")])
def test_count_reads_heavy_leaves(rfx, torch_mod, k, min_cov, heavy, monkeypatch):
    """RFX_HEAVY as test_heavy_leaf_slices_merge_exactly sets it: leaves of more than `heavy` records are left out of the main
    launch, counted in slices, and k_reduce_partials emits their survivors.  Proof that it emitted: stat_passes counts the main
    launch's passes only, each over at most `heavy` records of at most 16 windows, so m > stat_passes * heavy * 16 leaves
    survivors that only k_reduce_partials can have written; asserted below."""
    torch = torch_mod
    monkeypatch.setenv("RFX_HEAVY", heavy)
    b = base_for(rfx, torch, k)
    wk, wc, wd = b.want(k, min_cov)
    m = guard_band(torch, call_count_reads(rfx, b, k, min_cov), wk, wc, 1, torch.int32, where=f"heavy leaves k={k}")
    t = rfx.count_timing()
    print(f"k = {k}: m = {m}, main-launch passes = {t['stat_passes'][1]}")
    assert t["leaf"][1] >= 3, t                     # the main launch, the slices, the sort + k_reduce_partials
    assert m > t["stat_passes"][1] * int(heavy.split(",")[0]) * 16, (m, t)


def test_count_records_k31(rfx, torch_mod):
    """rfx_dev_count_records on the super-k-mer records rfx_dev_bucket_records_by_owner makes for one owner"""
    torch = torch_mod
    k = 31
    b = base_for(rfx, torch, k)
    doff = torch.empty(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    args = (b.dw.data_ptr(), b.n, b.wpr, b.L, k, 1)
    nrec, h = rfx.bucket_records_by_owner_dev(*args, 0, 0, doff.data_ptr())
    assert h is None and nrec > 0
    recs = torch.empty(2 * nrec, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nrec2, h = rfx.bucket_records_by_owner_dev(*args, recs.data_ptr(), nrec, doff.data_ptr())
    assert nrec2 == nrec and list(h) == [0, nrec]

    def call(pk, pc, cap):
        n, d = i64(0), i64(0)
        st = rfx.L.rfx_dev_count_records(rfx.ctx, ptr(recs.data_ptr()), i64(nrec), i64(len(b.km(k))), k, 2, BIG, O.TWIN_DS, ptr(pk), ptr(pc),
                                         i64(cap), C.byref(n), C.byref(d))
        return st, n.value
    wk, wc, wd = b.want(k, 2)
    guard_band(torch, call, wk, wc, 1, torch.int32, where="count_records")
    wrapper_need(torch, lambda pk, pc, cap: rfx.count_records_dev(recs.data_ptr(), nrec, len(b.km(k)), k, pk, pc, cap, 2), len(wk), 1)
    assert rfx.count_timing().get("leaf", (0, 0))[1] > 0


def test_count_wide_records_k63(rfx, torch_mod):
    """rfx_dev_count_wide_records on the 32-byte records rfx_dev_bucket_wide_records_by_owner makes for one owner (the
    wide-record leaf; its buffer holds WOBUF survivors, so m > stat_passes * WOBUF proves the direct write ran as well)"""
    torch = torch_mod
    k = 63
    b = base_for(rfx, torch, k)
    doff = torch.empty(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    args = (b.dw.data_ptr(), b.n, b.wpr, b.L, k, 1)
    nrec, h = rfx.bucket_wide_records_by_owner_dev(*args, 0, 0, doff.data_ptr())
    assert h is None and nrec > 0
    recs = torch.empty(4 * nrec, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nrec2, h = rfx.bucket_wide_records_by_owner_dev(*args, recs.data_ptr(), nrec, doff.data_ptr())
    assert nrec2 == nrec and list(h) == [0, nrec]

    def call(pk, pc, cap):
        n, d = i64(0), i64(0)
        st = rfx.L.rfx_dev_count_wide_records(rfx.ctx, ptr(recs.data_ptr()), i64(nrec), i64(len(b.km(k))), k, 2, BIG, ptr(pk), ptr(pc),
                                              i64(cap), C.byref(n), C.byref(d))
        return st, n.value
    wk, wc, wd = b.want(k, 2)
    m = guard_band(torch, call, wk, wc, 2, torch.int64, where="count_wide_records")
    t = rfx.count_timing()
    assert only_the_main_leaf_launch(t) and m > t["stat_passes"][1] * kernel_constants()[2], t
    wrapper_need(torch, lambda pk, pc, cap: rfx.count_wide_records_dev(recs.data_ptr(), nrec, len(b.km(k)), k, pk, pc, cap, 2), m, 2)


# ------------------------------------------------------------------ k > 31 on the bucketed path

@pytest.mark.parametrize("k,min_cov,wide_records", [(63, 2, None), (63, 1, None), (47, 2, "0"), (47, 2, "1"), (95, 2, None), (95, 1, None),
                                                    (127, 2, None)])
def test_count_reads_w_leaves(rfx, torch_mod, k, min_cov, wide_records, monkeypatch):
    """rfx_dev_count_reads_w on uniform reads: k = 63 and 47 (two-word leaves; k = 47 with RFX_WIDE_RECORDS forced each way),
    k = 95 and 127 (W-word leaves).  Proofs: the timing shows "leaf" and neither "count_w" nor "extract_w" (the bucketed
    path, not the sort path); the leaves buffer WOBUF survivors, so m > stat_passes * WOBUF means that both the flush and
    the wave-direct write ran; with RFX_WIDE_RECORDS the two plans differ in their leaf count at this size (16-byte elements
    are planned for 8192 per leaf, records for 6144: 16 against 32 leaves), which the k = 47 cases assert."""
    torch = torch_mod
    if wide_records is not None:
        monkeypatch.setenv("RFX_WIDE_RECORDS", wide_records)
    b = base_for(rfx, torch, k)
    wk, wc, wd = b.want(k, min_cov)
    m = guard_band(torch, call_count_reads_w(rfx, b, k, min_cov), wk, wc, k // 32 + 1, torch.int64, where=f"count_reads_w k={k}")
    t = rfx.count_timing()
    print(f"k = {k}: m = {m}, leaves = {t['stat_leaves'][1]}, passes = {t['stat_passes'][1]}")
    assert only_the_main_leaf_launch(t) and "count_w" not in t and "extract_w" not in t, t
    assert m > t["stat_passes"][1] * kernel_constants()[2], (m, t)
    if wide_records is not None:
        assert t["stat_leaves"][1] == (16 if wide_records == "0" else 32), t


@pytest.mark.parametrize("k", [63, 95])
def test_count_reads_ragged_w(rfx, torch_mod, k):
    """rfx_dev_count_reads_ragged_w: the uniform base reads with a length array"""
    torch = torch_mod
    b = base_for(rfx, torch, k)

    def call(pk, pc, cap):
        n, d, inst = i64(0), i64(0), i64(0)
        st = rfx.L.rfx_dev_count_reads_ragged_w(rfx.ctx, ptr(b.dw.data_ptr()), ptr(b.dl.data_ptr()), i64(b.n), b.wpr, b.L, k, 0, 0, 2, BIG,
                                                ptr(pk), ptr(pc), i64(cap), C.byref(n), C.byref(d), C.byref(inst))
        assert inst.value == len(b.km(k))
        return st, n.value
    wk, wc, wd = b.want(k, 2)
    m = guard_band(torch, call, wk, wc, k // 32 + 1, torch.int64, where=f"count_reads_ragged_w k={k}")
    t = rfx.count_timing()
    assert only_the_main_leaf_launch(t) and m > t["stat_passes"][1] * kernel_constants()[2], t


@pytest.mark.parametrize("k", [63, 95])
def test_count_wide_elems(rfx, torch_mod, k):
    """rfx_dev_count_wide_elems on the oracle's k-mers as AoS elements (k = 95: three-word elements)"""
    torch = torch_mod
    b = base_for(rfx, torch, k)
    km = b.km(k)
    de = torch.from_numpy(km.view(np.int64).reshape(-1).copy()).cuda()

    def call(pk, pc, cap):
        n, d = i64(0), i64(0)
        st = rfx.L.rfx_dev_count_wide_elems(rfx.ctx, ptr(de.data_ptr()), i64(len(km)), k, 2, BIG, ptr(pk), ptr(pc), i64(cap), C.byref(n),
                                            C.byref(d))
        return st, n.value
    wk, wc, wd = b.want(k, 2)
    m = guard_band(torch, call, wk, wc, k // 32 + 1, torch.int64, where=f"count_wide_elems k={k}")
    t = rfx.count_timing()
    assert only_the_main_leaf_launch(t) and m > t["stat_passes"][1] * kernel_constants()[2], t
    wrapper_need(torch, lambda pk, pc, cap: rfx.count_wide_elems_dev(de.data_ptr(), len(km), k, pk, pc, cap, 2), m, k // 32 + 1)


def test_count_reads_w_sort_path_k129(rfx, torch_mod):
    """k = 129 (W = 5) keeps the sort path, which knows the survivors before it emits: on RFX_E_CAP the whole buffer is
    untouched.  The timing shows "count_w" and "extract_w" and no "leaf"; asserted below."""
    torch = torch_mod
    k = 129
    b = base_for(rfx, torch, k)
    wk, wc, wd = b.want(k, 2)
    guard_band(torch, call_count_reads_w(rfx, b, k, 2), wk, wc, 5, torch.int64, untouched_on_cap=True, where="count_reads_w k=129")
    t = rfx.count_timing()
    assert "count_w" in t and "extract_w" in t and "leaf" not in t, t


# ------------------------------------------------------------------ pair_out: blocks of PBLOCK pairs and their hole fill

def combine(rfx, b, k, owners, scratch, out, cap, doff):
    m, inst = i64(0), i64(0)
    h = np.zeros(owners + 1, np.int64)
    st = rfx.L.rfx_dev_combine_reads(rfx.ctx, ptr(b.dw.data_ptr()), i64(b.n), b.wpr, b.L, k, 0, 0, owners, ptr(scratch.data_ptr()),
                                     ptr(out.data_ptr()), i64(cap), ptr(doff.data_ptr()), h.ctypes.data_as(C.c_void_p), C.byref(m),
                                     C.byref(inst))
    return st, m.value, h


@pytest.mark.parametrize("k", [31, 15])
def test_combine_reads(rfx, torch_mod, k):
    """rfx_dev_combine_reads: the leaves hand out blocks of PBLOCK pairs and fill the unused tails with holes, so the need
    includes block padding (need >= distinct).  Nothing at or past cap_pairs may be written in d_out_pairs (the scratch
    buffer is the callee's), and a retry with exactly the reported need gives every distinct k-mer with its count."""
    torch = torch_mod
    owners = 3
    b = base_for(rfx, torch, k)
    wk, wc, wd = b.want(k, 1)
    doff = torch.empty(owners + 1, dtype=torch.int64, device="cuda")
    probe = torch.empty(2 * 16, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st, need0, _ = combine(rfx, b, k, owners, probe, probe, 0, doff)
    assert st == E_CAP and need0 >= wd
    alloc = need0 + G
    scratch = torch.empty(2 * alloc, dtype=torch.int64, device="cuda")
    out = torch.empty(2 * alloc, dtype=torch.int64, device="cuda")

    def run(cap):
        out.view(torch.uint8).fill_(FILL); scratch.view(torch.uint8).fill_(FILL)
        torch.cuda.synchronize()
        r = combine(rfx, b, k, owners, scratch, out, cap, doff)
        torch.cuda.synchronize()
        return r

    def check_ok(cap):
        st, m, h = run(cap)
        assert (st, m) == (OK, wd) and h[0] == 0 and h[-1] == m, (cap, st, m, wd)
        bp = out[:2 * m].cpu().numpy().view(np.uint64).reshape(m, 2)
        order = np.argsort(bp[:, 0], kind="stable")
        assert np.array_equal(bp[order, 0], wk) and np.array_equal(bp[order, 1], wc.astype(np.uint64)), cap
        assert untouched(torch, out, 2 * cap), (cap, first_touched(torch, out.view(-1, 2), cap))

    for cap in (0, 1, wd // 2, wd - 1, wd, need0 - 1):
        st, need, _ = run(cap)
        assert st == E_CAP and wd <= need <= need0, (cap, st, need, need0, wd)
        assert untouched(torch, out, 2 * cap), (cap, first_touched(torch, out.view(-1, 2), cap))
        check_ok(need)
    check_ok(need0 + 1)
    assert need0 > wd                               # whole blocks: the unused tails were handed out too, and filled with holes


@pytest.mark.parametrize("k,heavy", [(31, None), (31, "40,16,64")])
def test_merge_pairs(rfx, torch_mod, k, heavy, monkeypatch):
    """rfx_dev_merge_pairs on every distinct k-mer's (k-mer, count) pair, twice over (the partial counts of two ranks): sums,
    then the coverage filter on the sum.  With RFX_HEAVY every leaf goes through the slices and k_reduce_partials sums the
    weighted partials (stat_passes counts the main launch only: m > stat_passes * heavy, asserted)."""
    torch = torch_mod
    b = base_for(rfx, torch, k)
    wk, wc, wd = b.want(k, 1)
    doff = torch.empty(2, dtype=torch.int64, device="cuda")
    probe = torch.empty(32, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st, need0, _ = combine(rfx, b, k, 1, probe, probe, 0, doff)
    assert st == E_CAP
    scratch = torch.empty(2 * need0, dtype=torch.int64, device="cuda"); pairs = torch.empty(2 * need0, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st, m, h = combine(rfx, b, k, 1, scratch, pairs, need0, doff)
    assert (st, m) == (OK, wd)
    twice = torch.cat([pairs[:2 * m], pairs[:2 * m]])
    if heavy:
        monkeypatch.setenv("RFX_HEAVY", heavy)

    def call(pk, pc, cap):
        n, d = i64(0), i64(0)
        st = rfx.L.rfx_dev_merge_pairs(rfx.ctx, ptr(twice.data_ptr()), i64(2 * m), k, 4, BIG, O.TWIN_DS, ptr(pk), ptr(pc), i64(cap), C.byref(n),
                                       C.byref(d))
        assert st != OK or d.value == wd
        return st, n.value
    keep = 2 * wc >= 4
    got = guard_band(torch, call, wk[keep], (2 * wc[keep]).astype(np.int32), 1, torch.int32, where=f"merge_pairs heavy={heavy}")
    t = rfx.count_timing()
    assert t.get("leaf", (0, 0))[1] > 0, t
    if heavy:
        assert t["leaf"][1] >= 3 and got > t["stat_passes"][1] * 40, (got, t)
    else:
        assert only_the_main_leaf_launch(t), t
    wrapper_need(torch, lambda pk, pc, cap: rfx.merge_pairs_dev(twice.data_ptr(), 2 * m, k, pk, pc, cap, 4), got, 1)


# ------------------------------------------------------------------ host entries: the copy comes after the check

def host_guard(call, want, width, dtype2=None, want2=None, where=""):
    """call(buf, buf2, cap) -> (status, n) on numpy buffers of need + G entries; on RFX_E_CAP both are wholly untouched"""
    need = len(want)
    want = np.ascontiguousarray(want).reshape(need, width)
    buf = np.empty((need + G, width), want.dtype)
    buf2 = np.empty(need + G, dtype2) if dtype2 is not None else None

    def run(cap):
        buf.view(np.uint8).fill(FILL)
        if buf2 is not None:
            buf2.view(np.uint8).fill(FILL)
        return call(buf, buf2, cap)

    def clean(a, lo):
        return a is None or bool((a[lo:].view(np.uint8) == FILL).all())

    for cap in (0, 1, need // 2, need - 1, need, need + 1):
        st, n = run(cap)
        if cap < need:
            assert (st, n) == (E_CAP, need), (where, cap, st, n, need)
            assert clean(buf, 0) and clean(buf2, 0), (where, cap)
            st, n = run(need)
        assert (st, n) == (OK, need), (where, cap, st, n)
        assert np.array_equal(buf[:need], want) and (buf2 is None or np.array_equal(buf2[:need], want2)), (where, cap)
        assert clean(buf, need) and clean(buf2, need), (where, cap)


@pytest.mark.parametrize("k", [31, 63, 129])
def test_host_extract_canon(rfx, k):
    """rfx_extract_canon / rfx_extract_canon_w on 600 of the base reads"""
    g = O.synth_genome(5, 20_000)
    L = 100 if k <= 31 else k + 40
    bases, off = O.synth_reads(5, g, 20_000, 0, 600, L)
    bases, off = np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(off, np.int64)
    want = O.extract_canon(bases, off, k) if k <= 31 else O.extract_canon_w(bases, off, k)
    fn = rfx.L.rfx_extract_canon if k <= 31 else rfx.L.rfx_extract_canon_w

    def call(buf, _, cap):
        n = i64(0)
        st = fn(rfx.ctx, bases.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), i64(len(off) - 1), k, 0, 0,
                buf.ctypes.data_as(C.c_void_p), i64(cap), C.byref(n))
        return st, n.value
    host_guard(call, want, 1 if k <= 31 else k // 32 + 1, where=f"extract_canon k={k}")


@pytest.mark.parametrize("k", [31, 63, 129])
def test_host_count_filter(rfx, torch_mod, k):
    """rfx_count_filter / rfx_count_filter_w on the oracle's k-mers of the base reads, min_cov 2"""
    b = base_for(rfx, torch_mod, k)
    km = np.ascontiguousarray(b.km(k))
    wk, wc, wd = b.want(k, 2)

    def call(buf, buf2, cap):
        n, d = i64(0), i64(0)
        if k <= 31:
            st = rfx.L.rfx_count_filter(rfx.ctx, km.ctypes.data_as(C.c_void_p), i64(len(km)), 2, BIG, O.TWIN_DS, buf.ctypes.data_as(C.c_void_p),
                                        buf2.ctypes.data_as(C.c_void_p), i64(cap), C.byref(n), C.byref(d))
        else:
            st = rfx.L.rfx_count_filter_w(rfx.ctx, km.ctypes.data_as(C.c_void_p), i64(len(km)), k, 2, BIG, buf.ctypes.data_as(C.c_void_p),
                                          buf2.ctypes.data_as(C.c_void_p), i64(cap), C.byref(n), C.byref(d))
        assert d.value == wd
        return st, n.value
    host_guard(call, wk, 1 if k <= 31 else k // 32 + 1, np.int32 if k <= 31 else np.int64, wc, where=f"count_filter k={k}")


# ------------------------------------------------------------------ the Python wrappers carry the need

def test_rfx_error_carries_the_need(rfx, torch_mod):
    """every RfxError raised for RFX_E_CAP has .need = the capacity to retry with: the four wrappers that count reads here, the
    other five (count_kmers_dev, count_records_dev, count_wide_records_dev, count_wide_elems_dev, merge_pairs_dev) in the tests
    of their entries (wrapper_need)"""
    torch = torch_mod
    from reflexiv_amd import RfxError
    for k in (31, 63):
        b = base_for(rfx, torch, k)
        wk, wc, wd = b.want(k, 2)
        W = 1 if k <= 31 else 2
        dk = torch.empty((len(wk) + G) * W, dtype=torch.int64, device="cuda"); dc = torch.empty(len(wk) + G, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        calls = ([lambda: rfx.count_reads_dev(b.dw.data_ptr(), b.n, b.wpr, b.L, k, dk.data_ptr(), dc.data_ptr(), 7, 2),
                  lambda: rfx.count_reads_ragged_dev(b.dw.data_ptr(), b.dl.data_ptr(), b.n, b.wpr, b.L, k, dk.data_ptr(), dc.data_ptr(), 7, 2)]
                 if k <= 31 else
                 [lambda: rfx.count_reads_w_dev(b.dw.data_ptr(), b.n, b.wpr, b.L, k, dk.data_ptr(), dc.data_ptr(), 7, 2),
                  lambda: rfx.count_reads_ragged_w_dev(b.dw.data_ptr(), b.dl.data_ptr(), b.n, b.wpr, b.L, k, dk.data_ptr(), dc.data_ptr(), 7, 2)])
        for f in calls:
            with pytest.raises(RfxError) as ei:
                f()
            assert ei.value.status == E_CAP and ei.value.need == len(wk)


# ------------------------------------------------------------------ the grow-and-retry loops

def two_step(bases, off, k, cover, P, max_cov=BIG):
    """the reference's route at k > 31: the counter's count and filter, then KmerBinarizer + the from-counts filter with the
    same bounds (the count read back as the CSV text would be: ten digits or more = 1000000000), then the driver.  kept =
    the k-mers that pass BOTH filters, those handed to the driver"""
    wk, wc, _ = O.count_filter_w(O.extract_canon_w(bases, off, k), k, cover, max_cov)
    asm = O.counter_to_asm_w(wk, k)
    cnt = np.minimum(wc, 1_000_000_000).astype(np.int32)
    keep = (cnt >= cover) & (cnt <= max_cov)
    text, nc, trace, _ = O.assemble_from_counts(asm[keep], cnt[keep], O.default_params(k=k, min_cov=cover, partitions=P, min_contig=100))
    return text, nc, trace, int(keep.sum())


@pytest.mark.parametrize("k", [31, 63])
def test_assemble_reads_grows_its_survivor_buffers(rfx, k, monkeypatch):
    """RFX_ASSEMBLE_KCAP = 1000 starts both count loops of rfx_assemble_reads below the survivors (asserted: kept > 1000), so
    the first count returns RFX_E_CAP and the loop retries with the reported need: text, contigs, trace and kept equal those
    of the call without the knob and the oracle's, the workspace is sane and a second call gives the same answer."""
    import reflexiv_amd
    g = O.synth_genome(5, 20_000)
    bases, off = O.synth_reads(5, g, 20_000, 0, 3000, 150)
    bases, off = np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(off, np.int64)
    prm = reflexiv_amd.default_params(k=k, min_cov=2, partitions=4, min_contig=100)
    plain = rfx.assemble_reads(bases, off, prm)
    monkeypatch.setenv("RFX_ASSEMBLE_KCAP", "1000")
    grown = rfx.assemble_reads(bases, off, prm)
    ws1 = rfx.workspace_bytes()
    again = rfx.assemble_reads(bases, off, prm)
    assert grown == plain and again == plain
    if k <= 31:
        wk, wc, wd = O.count_filter(O.extract_canon(bases, off, k), 2)
        assert plain[3] == len(wk)
        otext, onc, otrace, _ = O.assemble_from_counts(wk, wc, O.default_params(k=k, min_cov=2, partitions=4, min_contig=100))
        assert plain[:3] == (otext, onc, otrace)
    else:
        assert plain == two_step(bases, off, k, 2, 4)
    print(f"k = {k}: kept = {plain[3]}")
    assert plain[3] > 1000 and plain[1] > 0
    assert 0 < ws1 < 1 << 32 and rfx.workspace_bytes() == ws1          # the retries leave nothing behind that grows per call


def test_cli_counter_resident_grows_its_buffers(tmp_path):
    """`counter --resident -kmer 63` starts at max(65536, bases / 8) survivors: 6000 reads of 150 bases off a 200 kbp genome
    have more distinct 63-mers than that at minimum coverage 1 (asserted with the oracle), so its loop iterates; the output
    equals the non-resident counter's byte for byte"""
    host, k = host_bin(), 63
    g = O.synth_genome(41, 200_000)
    bases, off = O.synth_reads(41, g, 200_000, 0, 6000, 150)
    bases, off = np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(off, np.int64)
    wk, wc, wd = O.count_filter_w(O.extract_canon_w(bases, off, k), k, 1)
    print(f"distinct 63-mers: {wd}, first capacity: {max(65536, len(bases) // 8)}")
    assert len(wk) == wd and wd > max(65536, len(bases) // 8)
    fq = str(tmp_path / "r.fq")
    write_fq(fq, bases, off)
    plain, dev = str(tmp_path / "plain"), str(tmp_path / "dev")
    args = ["-fastq", fq, "-kmer", str(k), "-cover", "1"]
    subprocess.check_call([host, "counter", "-outfile", plain] + args, timeout=600)
    subprocess.check_call([host, "counter", "--resident", "-outfile", dev] + args, timeout=600)
    want = open(os.path.join(plain, f"Count_{k}", "part-00000.csv"), "rb").read()
    assert want.count(b"\n") >= wd
    assert open(os.path.join(dev, f"Count_{k}", "part-00000.csv"), "rb").read() == want


# ------------------------------------------------------------------ device record operators: rfx_records promises "nothing written"

class DevRecs:
    """a record set in HBM behind an rfx_records: the arrays carry `guard` spare entries each (0 for inputs)"""

    def __init__(self, torch, n, words, kw, guard=0):
        from reflexiv_amd._lib import CRecords
        self.torch, self.n, self.words, self.kw = torch, n, words, kw
        i64t, i32t = torch.int64, torch.int32
        self.arr = {"key": torch.empty((n + guard) * kw, dtype=i64t, device="cuda"), "marker": torch.empty(n + guard, dtype=i32t, device="cuda"),
                    "ext_off": torch.empty(n + 1 + guard, dtype=i64t, device="cuda"), "ext": torch.empty(max(1, words) + guard, dtype=i64t, device="cuda"),
                    "left": torch.empty(n + guard, dtype=i32t, device="cuda"), "right": torch.empty(n + guard, dtype=i32t, device="cuda")}
        self.CRecords = CRecords

    @staticmethod
    def of(torch, r, kw):
        d = DevRecs(torch, r.n, int(r.ext_off[r.n]), kw)
        d.arr["key"].copy_(torch.from_numpy(np.ascontiguousarray(r.key, np.uint64).reshape(-1).view(np.int64).copy()))
        d.arr["ext_off"].copy_(torch.from_numpy(np.ascontiguousarray(r.ext_off, np.int64)))
        if d.words:
            d.arr["ext"][:d.words].copy_(torch.from_numpy(np.ascontiguousarray(r.ext, np.uint64).view(np.int64).copy()))
        for f in ("marker", "left", "right"):
            d.arr[f].copy_(torch.from_numpy(np.ascontiguousarray(getattr(r, f), np.int32)))
        torch.cuda.synchronize()
        return d

    def c(self, cap_n=None, cap_words=None):
        c = self.CRecords()
        c.n, c.need_words, c.key_words = self.n, self.words, self.kw
        for f, t in self.arr.items():
            setattr(c, f, t.data_ptr())
        c.cap_n = self.n if cap_n is None else cap_n
        c.cap_words = self.words if cap_words is None else cap_words
        return c

    def fill(self):
        for t in self.arr.values():
            t.view(self.torch.uint8).fill_(FILL)

    def untouched_from(self, n, words):
        """nothing written at or past n records / words (n = words = 0: anywhere)"""
        start = {"key": n * self.kw, "marker": n, "ext_off": n + 1 if n or words else 0, "ext": words, "left": n, "right": n}
        return [f for f, t in self.arr.items() if not untouched(self.torch, t, start[f])]

    def equals(self, r):
        n, w = r.n, int(r.ext_off[r.n])
        a = {f: t.cpu().numpy() for f, t in self.arr.items()}
        return (np.array_equal(a["key"][:n * self.kw].view(np.uint64), np.ascontiguousarray(r.key, np.uint64).reshape(-1))
                and np.array_equal(a["ext_off"][:n + 1], r.ext_off) and np.array_equal(a["ext"][:w].view(np.uint64), r.ext[:w])
                and all(np.array_equal(a[f][:n], getattr(r, f)) for f in ("marker", "left", "right")))


def records_guard(torch, call, want, kw, want_ps=None, where=""):
    """call(c_out, ps_ptr) -> status.  cap_n and cap_words exact and one short, each independently: on RFX_E_CAP need_n and
    need_words are the oracle operator's sizes and every output array (the partition starts too) is wholly untouched; on
    the exact fit the records equal the oracle's and the guard entries are intact."""
    need_n, need_w = want.n, int(want.ext_off[want.n])
    assert need_n > 1 and need_w > 1
    out = DevRecs(torch, need_n, need_w, kw, guard=G)
    ps = torch.empty((0 if want_ps is None else len(want_ps)) + G, dtype=torch.int64, device="cuda")
    for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1), (need_n - 1, need_w - 1), (need_n, need_w)):
        out.fill(); ps.view(torch.uint8).fill_(FILL)
        torch.cuda.synchronize()
        c = out.c(cap_n, cap_w)
        c.n, c.need_words, c.need_n = -7, -7, -7
        st = call(c, ps.data_ptr())
        torch.cuda.synchronize()
        assert (int(c.need_n), int(c.need_words)) == (need_n, need_w), (where, cap_n, cap_w, int(c.need_n), int(c.need_words), need_n, need_w)
        if (cap_n, cap_w) != (need_n, need_w):
            assert st == E_CAP, (where, cap_n, cap_w, st)
            assert out.untouched_from(0, 0) == [] and untouched(torch, ps), (where, cap_n, cap_w, out.untouched_from(0, 0))
        else:
            assert st == OK and int(c.n) == need_n and int(c.key_words) in (kw, 0 if kw == 1 else kw), (where, st, int(c.n))
            assert out.equals(want), where
            assert out.untouched_from(need_n, need_w) == [], (where, out.untouched_from(need_n, need_w))
            if want_ps is not None:
                assert np.array_equal(ps[:len(want_ps)].cpu().numpy(), want_ps) and untouched(torch, ps, len(want_ps)), where


@pytest.fixture(scope="module")
def planted(golden_dir):
    return np.load(os.path.join(golden_dir, "planted.npz"))


@pytest.mark.parametrize("k", [31, 63, 65])
def test_device_record_operators(rfx, torch_mod, planted, k):
    """rfx_dev_rc_expand_subkmer, rfx_dev_sort_records, rfx_dev_fork_filter (forward and reflected) and rfx_dev_extend_pass
    (stage 0 on one-word extensions, stage 2 on the tenth pass, when records and extension words differ in number) on the
    planted fixture: k = 31 (one-word keys), k = 63 and 65 (two- and three-word keys)"""
    torch = torch_mod
    from reflexiv_amd.api import sub_words
    P, min_err, twin = 4, 8, O.TWIN_DS
    kw = sub_words(k)
    if k == 31:
        keys, counts = planted["k31_keys"], planted["k31_counts"]
    else:
        wk, wc, _ = O.count_filter_w(O.extract_canon_w(planted["bases"], planted["read_off"], k), k, 2)
        keys, counts = O.counter_to_asm_w(wk, k), wc.astype(np.int32)
    n = len(counts)
    dkm = torch.from_numpy(np.ascontiguousarray(keys, np.uint64).reshape(-1).view(np.int64).copy()).cuda()
    dcn = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
    L, ctx = rfx.L, rfx.ctx
    o1 = O.rc_expand_subkmer(keys, counts, k)
    records_guard(torch, lambda c, ps: L.rfx_dev_rc_expand_subkmer(ctx, ptr(dkm.data_ptr()), ptr(dcn.data_ptr()), i64(n), k, C.byref(c)),
                  o1, kw, where=f"rc_expand k={k}")

    def sort_case(r, where):
        s = O.sort_records(r)
        sps = O.partition_starts(s.key, P)
        din = DevRecs.of(torch, r, kw)
        ci = din.c()
        records_guard(torch, lambda c, ps: L.rfx_dev_sort_records(ctx, C.byref(ci), P, k, C.byref(c), ptr(ps)), s, kw, sps, where=where)
        return s, sps

    def fork_case(reflected, r, rps, where):
        want, wps = (O.fork_filter_reflected if reflected else O.fork_filter_forward)(r, rps, k, min_err, twin)
        din = DevRecs.of(torch, r, kw)
        ci = din.c()
        dps = torch.from_numpy(np.ascontiguousarray(rps, np.int64)).cuda()
        records_guard(torch, lambda c, ps: L.rfx_dev_fork_filter(ctx, reflected, C.byref(ci), ptr(dps.data_ptr()), P, k, min_err, twin,
                                                                 C.byref(c), ptr(ps)), want, kw, wps, where=where)
        return want, wps

    o2, ps2 = sort_case(o1, f"sort k={k}")
    o3, ps3 = fork_case(0, o2, ps2, f"fork forward k={k}")
    o4 = O.sort_records(O.reflect_from_forward(o3, k))
    ps4 = O.partition_starts(o4.key, P)
    o5, ps5 = fork_case(1, o4, ps4, f"fork reflected k={k}")
    cur = O.random_reflection(o5, ps5, k)
    for i in range(10):
        cur = O.sort_records(cur)
        cps = O.partition_starts(cur.key, P)
        nxt, nps = O.extend_pass(cur, cps, k, twin)
        stage = 0 if i < 4 else (1 if i == 4 else 2)
        if i in (0, 9):
            din = DevRecs.of(torch, cur, kw)
            ci = din.c()
            dps = torch.from_numpy(np.ascontiguousarray(cps, np.int64)).cuda()
            records_guard(torch, lambda c, ps: L.rfx_dev_extend_pass(ctx, C.byref(ci), ptr(dps.data_ptr()), P, k, twin, stage, 2, C.byref(c),
                                                                     ptr(ps)), nxt, kw, nps, where=f"extend pass {i} k={k}")
        if i == 9:
            assert int(nxt.ext_off[nxt.n]) > nxt.n         # records and extension words differ: the two capacities are two things
        cur = nxt


# ------------------------------------------------------------------ the dynamic-k records and the contig de-duplication (host buffers)

def dyn_guard(rfx, fn_call, want, where):
    """fn_call(c_out) -> status on rfx_dyn_records outputs with G guard entries: cap_n, cap_key and cap_ext one short, each
    alone -> RFX_E_CAP with n / need_key / need_ext = the oracle's sizes and every record array untouched; the exact fit
    equals the oracle and leaves the guard alone"""
    from reflexiv_amd._lib import CDynRecords
    n, nk, ne = want.n, int(want.key_off[-1]), int(want.ext_off[-1])
    assert n > 1 and nk > 1 and ne > 1
    arr = {"key": np.empty(nk + G, np.uint8), "key_off": np.empty(n + 1 + G, np.int64), "ext": np.empty(ne + G, np.uint8),
           "ext_off": np.empty(n + 1 + G, np.int64), "marker": np.empty(n + G, np.int32), "left": np.empty(n + G, np.int32),
           "right": np.empty(n + G, np.int32)}

    def clean(start):
        return [f for f, a in arr.items() if not (a[start[f]:].view(np.uint8) == FILL).all()]

    for cn, ck, ce in ((n - 1, nk, ne), (n, nk - 1, ne), (n, nk, ne - 1), (n, nk, ne)):
        c = CDynRecords()
        for f, a in arr.items():
            a.view(np.uint8).fill(FILL)
            setattr(c, f, a.ctypes.data)
        c.n, c.need_key, c.need_ext = -7, -7, -7
        c.cap_n, c.cap_key, c.cap_ext = cn, ck, ce
        st = fn_call(c)
        assert (int(c.n), int(c.need_key), int(c.need_ext)) == (n, nk, ne), (where, cn, ck, ce, int(c.n), int(c.need_key), int(c.need_ext))
        if (cn, ck, ce) != (n, nk, ne):
            assert st == E_CAP and clean(dict.fromkeys(arr, 0)) == [], (where, cn, ck, ce, st)
        else:
            assert st == OK, (where, st)
            assert np.array_equal(arr["key"][:nk], want.key) and np.array_equal(arr["ext"][:ne], want.ext), where
            assert np.array_equal(arr["key_off"][:n + 1], want.key_off) and np.array_equal(arr["ext_off"][:n + 1], want.ext_off), where
            assert all(np.array_equal(arr[f][:n], getattr(want, f)) for f in ("marker", "left", "right")), where
            assert clean({"key": nk, "key_off": n + 1, "ext": ne, "ext_off": n + 1, "marker": n, "left": n, "right": n}) == [], where


def test_dynamic_k_record_capacities(rfx):
    """rfx_dyn_sort and rfx_dyn_extend_pass on the first reference-made case of tests/golden/dynamic_vectors.npz"""
    from reflexiv_amd.api import DynRecords
    from tests.test_oracle_dynamic import VEC, cases, rows_of
    z = np.load(VEC)
    case = cases()[0]
    P = int(z[case + "/meta"][0])
    rows = rows_of(z, case + "/random_reflection")
    r = DynRecords.from_rows(rows)
    o = O.dyn_sort(O.dyn_binarize_rows(rows))
    ops = O.dyn_partition_starts(o, P)
    ci = r._c()
    ps = np.empty(P + 1, np.int64)
    dyn_guard(rfx, lambda c: rfx.L.rfx_dyn_sort(rfx.ctx, C.byref(ci), P, C.byref(c), ps.ctypes.data_as(C.c_void_p)), o, "dyn_sort")
    assert np.array_equal(ps, ops)
    want, wps = O.dyn_extend_pass(o, ops, 0)
    s = DynRecords(o.key, o.key_off, o.ext, o.ext_off, o.marker, o.left, o.right)
    cs = s._c()
    gps = np.empty(P + 1, np.int64)
    dyn_guard(rfx, lambda c: rfx.L.rfx_dyn_extend_pass(rfx.ctx, C.byref(cs), ops.ctypes.data_as(C.c_void_p), P, 0, 5, 2, C.byref(c),
                                                       gps.ctypes.data_as(C.c_void_p)), want, "dyn_extend_pass")
    assert np.array_equal(gps, wps)


def test_dedup_contigs_capacities(rfx):
    """rfx_dedup_contigs with cap_bases, cap_contigs and text_cap one short, each alone: RFX_E_CAP with *out_n (and *text_len)
    reported; a short survivor capacity leaves out_bases and out_off untouched; a short text_cap may fill the text below it,
    nothing at or past it changes; the exact fit equals the oracle"""
    rng = np.random.default_rng(4)
    comp = str.maketrans("ACGT", "TGCA")
    seqs = ["".join("ACGT"[b] for b in rng.integers(0, 4, int(L))) for L in (900, 1500, 700, 2500, 640)]
    contigs = [seqs[0], seqs[1].translate(comp)[::-1], seqs[2], seqs[1], seqs[3], seqs[0].translate(comp)[::-1], seqs[4]]
    want = O.dedup_contigs(contigs, 500)
    surv, text = want["rounds"][2], want["text"]
    off = np.zeros(len(contigs) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in contigs])
    bases = np.frombuffer("".join(contigs).encode(), np.uint8).copy()
    nb, m, tl = sum(len(s) for s in surv), len(surv), len(text)
    assert 0 < m < len(contigs) and tl > nb
    ob, oo, tb = np.empty(nb + G, np.uint8), np.empty(m + 1 + G, np.int64), np.empty(tl + G, np.uint8)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    for cb, cc, tc in ((nb - 1, m, tl), (nb, m - 1, tl), (nb, m, tl - 1), (nb, m, tl)):
        for a in (ob, oo, tb):
            a.view(np.uint8).fill(FILL)
        on, tlen = i64(-7), i64(-7)
        rn = (C.c_int64 * 3)()
        st = rfx.L.rfx_dedup_contigs(rfx.ctx, hp(bases), hp(off), i64(len(contigs)), 500, hp(ob), i64(cb), hp(oo), i64(cc), C.byref(on),
                                     hp(tb), i64(tc), C.byref(tlen), rn)
        assert (on.value, tlen.value) == (m, tl), (cb, cc, tc, on.value, tlen.value)
        assert (tb[tc:] == FILL).all(), (cb, cc, tc)
        if (cb, cc) != (nb, m):
            assert st == E_CAP and (ob == FILL).all() and (oo.view(np.uint8) == FILL).all(), (cb, cc, tc, st)
        else:
            assert st == (OK if tc == tl else E_CAP), (cb, cc, tc, st)
            assert [bytes(ob[oo[i]:oo[i + 1]]).decode() for i in range(m)] == surv
            assert (ob[nb:] == FILL).all() and (oo[m + 1:].view(np.uint8) == FILL).all()
        if tc == tl:
            assert bytes(tb[:tl]).decode() == text


def test_contigs_text_fills_its_buffer_up_to_cap(rfx, planted):
    """rfx_contigs_text (the formatter every driver ends with) clips: with a short cap it reports the length needed and fills
    the buffer up to cap (those bytes are unspecified) -- nothing at or past cap changes; the exact cap gives the oracle's text"""
    from reflexiv_amd.api import as_records
    r = O.Records(*(planted[f"k31_ds_pass5_{f}"] for f in ("key", "marker", "ext_off", "ext", "left", "right")))
    text, nc = O.contigs_text(r, 31, 40, O.TWIN_DS)
    need = len(text)
    assert nc > 0 and need > 1000
    rr = as_records(r)
    ci = rr._c()
    buf = np.empty(need + G, np.uint8)
    for cap in (0, 1, need // 2, need - 1, need, need + 1):
        buf.fill(FILL)
        ln, n = i64(-7), i64(-7)
        st = rfx.L.rfx_contigs_text(rfx.ctx, C.byref(ci), 31, 40, O.TWIN_DS, buf.ctypes.data_as(C.c_void_p), i64(cap), C.byref(ln), C.byref(n))
        assert (st, ln.value, n.value) == (E_CAP if cap < need else OK, need, nc), (cap, st, ln.value, n.value)
        assert (buf[min(cap, need):] == FILL).all(), cap
        if cap >= need:
            assert bytes(buf[:need]).decode() == text, cap
