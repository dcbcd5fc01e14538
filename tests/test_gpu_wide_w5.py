"""Five- to eight-word k-mers (k = 129..255, not a multiple of 32) stay on the sort path of rfx_wide.hip (extract_w, an LSD
sort word by word -- the last word over 2 * (k % 32) key bits, 2 bits at k = 129 --, k_heads_w / k_starts_w / k_keep_w /
k_emit_w): rfx_extract_canon_w, rfx_count_filter_w and rfx_dev_count_reads_w against the oracle's k > 31 counter.  And the
refusals of every count entry: k = 32, 64, 96, 128, 160, 256 and beyond, each entry's own upper bound, reads wider than their
words, negative clips -- RFX_E_ARG before anything is launched or written.  Bit-exact (integer work)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_ragged_w import upload

pytestmark = pytest.mark.gpu

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "n": "n", "a": "t", "c": "g", "g": "c", "t": "a"}
KS = [129, 159, 161, 223, 255]
FILL = 0xA5
OK, E_ARG, E_CAP = 0, -1, -2
BIG = 10_000_000


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


def reads_of(strings):
    bases = np.frombuffer("".join(strings).encode(), np.uint8).copy()
    off = np.cumsum([0] + [len(r) for r in strings]).astype(np.int64)
    return bases, off


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def ragged_reads_w5(seed, k, n_reads=500, genome_len=4000):
    """seeded reads of the edge lengths around k, the multiples of 32 near it, k + 60, and random lengths up to k + 60, with N,
    lower case and reverse-complemented reads; deep enough (~25x) that min_cov 2 keeps k-mers and max_cov 4 drops some"""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), size=genome_len))
    m32 = 32 * (k // 32)
    edge = [0, 1, k - 1, k, k + 1, m32, m32 + 32, m32 + 64, k + 31, k + 32, k + 33, k + 60]
    reads = []
    for i in range(n_reads):
        L = edge[i % len(edge)] if i < 4 * len(edge) else int(rng.integers(k - 3, k + 61))
        p = int(rng.integers(0, genome_len - L))
        s = list(genome[p:p + L])
        if L and rng.random() < 0.05:
            s[int(rng.integers(0, L))] = "N"
        if L and rng.random() < 0.05:
            j = int(rng.integers(0, L))
            s[j] = s[j].lower()
        s = "".join(s)
        reads.append(revcomp(s) if rng.random() < 0.5 else s)
    return reads_of(reads)


_cache = {}


def ragged_case(k):
    if k not in _cache:
        bases, off = ragged_reads_w5(3000 + k, k)
        _cache[k] = (bases, off, O.extract_canon_w(bases, off, k))
    return _cache[k]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("clips", [(0, 0), (3, 5)])
def test_extraction_matches_the_oracle(rfx, k, clips):
    bases, off, km0 = ragged_case(k)
    want = km0 if clips == (0, 0) else O.extract_canon_w(bases, off, k, *clips)
    got = rfx.ReverseComplementKmerBinaryExtractionFromDataset64(bases, off, k, *clips)
    assert len(want) > 1000 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("k", KS)
def test_count_filter_matches_the_oracle(rfx, k):
    """min_cov 1 and 2, and max_cov 4 (both filters of the counter); some k-mers must pass and some fall to each filter"""
    bases, off, km = ragged_case(k)
    W = k // 32 + 1
    sizes = []
    for min_cov, max_cov in ((1, BIG), (2, BIG), (1, 4)):
        keys, counts, nd = rfx.groupBy_count_filter_w(km, k, min_cov, max_cov)
        wk, wc, wd = O.count_filter_w(km, k, min_cov, max_cov)
        assert nd == wd and np.array_equal(np.asarray(keys).reshape(-1, W), wk) and np.array_equal(np.asarray(counts), wc), (k, min_cov, max_cov)
        sizes.append(len(wk))
    assert 0 < sizes[1] < sizes[0] and 0 < sizes[2] < sizes[0], sizes


@pytest.mark.parametrize("k", KS)
def test_uniform_count_runs_the_sort_path(rfx, torch_mod, k):
    """count_reads_w_dev at W >= 5: the timing shows "extract_w" and "count_w" and no "leaf" -- the mirror of
    test_uniform_count_runs_the_leaf_kernels"""
    torch = torch_mod
    Gn, n, L = 20_000, 2000, k + 40
    og = O.synth_genome(17, Gn)
    bases, off = O.synth_reads(17, og, Gn, 0, n, L)
    bases, off = np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(off, np.int64)
    dw, dl, nn, wpr, maxlen = upload(rfx, torch, bases, off)
    W = k // 32 + 1
    cap = rfx.kmers_per_read_w(L, k) * n
    assert cap == 41 * n
    dk = torch.empty(cap * W, dtype=torch.int64, device="cuda"); dc = torch.empty(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    km = O.extract_canon_w(bases, off, k)
    for min_cov in (1, 2):
        m, nd, inst = rfx.count_reads_w_dev(dw.data_ptr(), n, wpr, L, k, dk.data_ptr(), dc.data_ptr(), cap, min_cov)
        t = rfx.count_timing()
        assert t.get("count_w", (0, 0))[1] > 0 and t.get("extract_w", (0, 0))[1] > 0 and "leaf" not in t, t
        wk, wc, wd = O.count_filter_w(km, k, min_cov)
        assert (m, nd, inst) == (len(wk), wd, cap) and m > 0
        assert np.array_equal(dk[:W * m].cpu().numpy().view(np.uint64).reshape(m, W), wk)
        assert np.array_equal(dc[:m].cpu().numpy(), wc)


@pytest.mark.parametrize("k", [130, 254])
def test_palindromic_windows(rfx, k):
    """a window that equals its own reverse complement exists only at an even k: h + revcomp(h).  Forward == reverse
    complement, the tie goes to forward, and the k-mer counts once per occurrence on either strand."""
    rng = np.random.default_rng(k)
    reads = []
    for i in range(6):
        h = "".join(rng.choice(list("ACGT"), size=k // 2))
        pal = h + revcomp(h)
        assert pal == revcomp(pal)
        flank = "".join(rng.choice(list("ACGT"), size=20))
        r = flank[:10] + pal + flank[10:]
        reads += [pal, r, revcomp(r)][:1 + i % 3] * (1 + i % 2)
    bases, off = reads_of(reads)
    want = O.extract_canon_w(bases, off, k)
    got = rfx.ReverseComplementKmerBinaryExtractionFromDataset64(bases, off, k)
    assert np.array_equal(got, want)
    keys, counts, nd = rfx.groupBy_count_filter_w(got, k, 1)
    wk, wc, wd = O.count_filter_w(want, k, 1)
    assert nd == wd and np.array_equal(np.asarray(keys).reshape(wk.shape), wk) and np.array_equal(np.asarray(counts), wc)
    assert wc.max() >= 2


@pytest.mark.parametrize("k", KS)
def test_kmers_that_differ_only_in_the_last_word(rfx, torch_mod, k):
    """reads of exactly k bases that share their first 32 * (W - 1) bases: every k-mer differs from the others in the last
    word only (k = 129: in its 2 bits), so the whole order rests on the sort's first pass over 2 * (k % 32) key bits.  The
    shared part starts with AAAA and the k-mers do not end in TTTT, so the forward strand is the canonical one."""
    torch = torch_mod
    W, res = k // 32 + 1, k % 32
    rng = np.random.default_rng(k)
    head = "AAAA" + "".join(rng.choice(list("ACGT"), size=32 * (W - 1) - 5)) + "C"
    if res == 1:
        tails = list("ACGT")
    else:
        tails = sorted({"".join(rng.choice(list("ACGT"), size=res - 1)) + "ACG"[i % 3] for i in range(300)})
    reads = []
    for i, t in enumerate(tails):
        reads += [head + t] * (1 + (i * 7) % 5)
    order = rng.permutation(len(reads))
    bases, off = reads_of([reads[i] for i in order])
    km = O.extract_canon_w(bases, off, k)
    assert len(km) == len(reads) and len(np.unique(km[:, :W - 1], axis=0)) == 1 and len(np.unique(km[:, W - 1])) == len(tails)
    got = rfx.ReverseComplementKmerBinaryExtractionFromDataset64(bases, off, k)
    assert np.array_equal(got, km)
    for min_cov, max_cov in ((1, BIG), (2, BIG), (1, 4)):
        keys, counts, nd = rfx.groupBy_count_filter_w(km, k, min_cov, max_cov)
        wk, wc, wd = O.count_filter_w(km, k, min_cov, max_cov)
        assert nd == wd == len(tails) and len(wk) > 0
        assert np.array_equal(np.asarray(keys).reshape(-1, W), wk) and np.array_equal(np.asarray(counts), wc)
    # the same reads through the device entry (uniform reads of k bases: one window each)
    dw, dl, n, wpr, maxlen = upload(rfx, torch, bases, off)
    dk = torch.empty(n * W, dtype=torch.int64, device="cuda"); dc = torch.empty(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m, nd, inst = rfx.count_reads_w_dev(dw.data_ptr(), n, wpr, k, k, dk.data_ptr(), dc.data_ptr(), n, 1)
    wk, wc, wd = O.count_filter_w(km, k, 1)
    assert (m, nd, inst) == (len(wk), wd, n)
    assert np.array_equal(dk[:W * m].cpu().numpy().view(np.uint64).reshape(m, W), wk) and np.array_equal(dc[:m].cpu().numpy(), wc)


# ------------------------------------------------------------------ refusals

def i64(v):
    return C.c_int64(int(v))


class Scratch:
    """device and host buffers filled with 0xA5, and sentinels in every scalar output: a refused call leaves all of them alone"""
    SENT = -77

    def __init__(self, torch):
        self.torch = torch
        self.words = torch.zeros(64 * 8, dtype=torch.int64, device="cuda")                 # 64 reads of 8 words
        self.lens = torch.full((64,), 200, dtype=torch.int32, device="cuda")
        self.dk = torch.empty(8 * 4096, dtype=torch.int64, device="cuda")
        self.dc = torch.empty(4096, dtype=torch.int64, device="cuda")
        self.doff = torch.empty(65, dtype=torch.int64, device="cuda")
        self.hk = np.empty(8 * 4096, np.uint64)
        self.hc = np.empty(4096, np.int64)
        self.hoff = np.empty(65, np.int64)
        self.refill()

    def refill(self):
        for t in (self.dk, self.dc, self.doff):
            t.view(self.torch.uint8).fill_(FILL)
        for a in (self.hk, self.hc, self.hoff):
            a.view(np.uint8).fill(FILL)
        self.torch.cuda.synchronize()
        self.n, self.d, self.inst = i64(self.SENT), i64(self.SENT), i64(self.SENT)

    def untouched(self):
        self.torch.cuda.synchronize()
        dev = all(bool((t.view(self.torch.uint8) == FILL).all()) for t in (self.dk, self.dc, self.doff))
        host = all(bool((a.view(np.uint8) == FILL).all()) for a in (self.hk, self.hc, self.hoff))
        return dev and host and (self.n.value, self.d.value, self.inst.value) == (self.SENT,) * 3


@pytest.fixture(scope="module")
def scratch(torch_mod):
    return Scratch(torch_mod)


READS = np.frombuffer(b"ACGT" * 100, np.uint8).copy()
READ_OFF = np.array([0, 400], np.int64)
COUNT_W = ("rfx_extract_canon_w", "rfx_count_filter_w", "rfx_dev_count_reads_w", "rfx_dev_count_reads_ragged_w", "rfx_dev_count_wide_elems",
           "rfx_dev_order_kmers_w")


def entries(rfx, s, k, front_clip=0, end_clip=0, wpr=8, read_len=200):
    """every entry that takes a k, on the scratch buffers -> {name: thunk that returns the status}.  Outputs: s.dk / s.dc /
    s.doff (device), s.hk / s.hc / s.hoff (host), s.n / s.d / s.inst."""
    p = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    L, ctx = rfx.L, rfx.ctx
    km = np.zeros(8 * 16, np.uint64)
    reads = (p(s.words), i64(64), wpr, read_len, k, front_clip, end_clip)
    return {
        # k > 31
        "rfx_extract_canon_w": lambda: L.rfx_extract_canon_w(ctx, hp(READS), hp(READ_OFF), i64(1), k, front_clip, end_clip, hp(s.hk), i64(4096),
                                                             C.byref(s.n)),
        "rfx_count_filter_w": lambda: L.rfx_count_filter_w(ctx, hp(km), i64(16), k, 1, BIG, hp(s.hk), hp(s.hc), i64(4096), C.byref(s.n),
                                                           C.byref(s.d)),
        "rfx_dev_count_reads_w": lambda: L.rfx_dev_count_reads_w(ctx, *reads, 1, BIG, p(s.dk), p(s.dc), i64(4096), C.byref(s.n), C.byref(s.d),
                                                                 C.byref(s.inst)),
        "rfx_dev_count_reads_ragged_w": lambda: L.rfx_dev_count_reads_ragged_w(ctx, p(s.words), p(s.lens), i64(64), wpr, read_len, k, front_clip,
                                                                               end_clip, 1, BIG, p(s.dk), p(s.dc), i64(4096), C.byref(s.n),
                                                                               C.byref(s.d), C.byref(s.inst)),
        "rfx_dev_count_wide_elems": lambda: L.rfx_dev_count_wide_elems(ctx, p(s.words), i64(16), k, 1, BIG, p(s.dk), p(s.dc), i64(4096),
                                                                       C.byref(s.n), C.byref(s.d)),
        "rfx_dev_order_kmers_w": lambda: L.rfx_dev_order_kmers_w(ctx, p(s.dk), p(s.dc), i64(16), k),
        "rfx_dev_count_wide_records": lambda: L.rfx_dev_count_wide_records(ctx, p(s.words), i64(16), i64(0), k, 1, BIG, p(s.dk), p(s.dc),
                                                                           i64(4096), C.byref(s.n), C.byref(s.d)),
        "rfx_dev_bucket_wide_by_owner": lambda: L.rfx_dev_bucket_wide_by_owner(ctx, *reads, 2, p(s.dk), i64(4096), p(s.doff), hp(s.hoff)),
        "rfx_dev_bucket_wide_records_by_owner": lambda: L.rfx_dev_bucket_wide_records_by_owner(ctx, *reads, 2, p(s.dk), i64(4096), p(s.doff),
                                                                                               hp(s.hoff), C.byref(s.n)),
        # k <= 31
        "rfx_extract_canon": lambda: L.rfx_extract_canon(ctx, hp(READS), hp(READ_OFF), i64(1), k, front_clip, end_clip, hp(s.hk), i64(4096),
                                                         C.byref(s.n)),
        "rfx_dev_count_reads": lambda: L.rfx_dev_count_reads(ctx, *reads, 1, BIG, 0, None, i64(0), p(s.dk), p(s.dc), i64(4096), C.byref(s.n),
                                                             C.byref(s.d), C.byref(s.inst)),
        "rfx_dev_count_reads_ragged": lambda: L.rfx_dev_count_reads_ragged(ctx, p(s.words), p(s.lens), i64(64), wpr, read_len, k, front_clip,
                                                                           end_clip, 1, BIG, 0, p(s.dk), p(s.dc), i64(4096), C.byref(s.n),
                                                                           C.byref(s.d), C.byref(s.inst)),
        "rfx_dev_combine_reads": lambda: L.rfx_dev_combine_reads(ctx, *reads, 2, p(s.dk), p(s.dk), i64(2048), p(s.doff), hp(s.hoff), C.byref(s.n),
                                                                 C.byref(s.inst)),
        "rfx_dev_bucket_by_owner": lambda: L.rfx_dev_bucket_by_owner(ctx, *reads, 2, p(s.dk), i64(4096), p(s.doff), hp(s.hoff)),
        "rfx_dev_bucket_records_by_owner": lambda: L.rfx_dev_bucket_records_by_owner(ctx, *reads, 2, p(s.dk), i64(4096), p(s.doff), hp(s.hoff),
                                                                                     C.byref(s.n)),
    }


def refused(rfx, s, names, k, **kw):
    """after a refill, ONLY the named entries are called: each returns RFX_E_ARG, and every buffer and scalar output is as it was"""
    s.refill()
    e = entries(rfx, s, k, **kw)
    st = {nm: e[nm]() for nm in names}
    assert all(v == E_ARG for v in st.values()), (k, kw, st)
    assert s.untouched(), (k, kw, names)


@pytest.mark.parametrize("k", [32, 64, 96, 128, 160, 256, 257])
def test_w_entries_refuse_a_k_out_of_range(rfx, scratch, k):
    """a multiple of 32 has no last word, k > 255 more than eight words: RFX_E_ARG from every k > 31 entry, with the buffers,
    *out_n, *out_distinct and *out_instances as they were"""
    refused(rfx, scratch, COUNT_W + ("rfx_dev_count_wide_records", "rfx_dev_bucket_wide_by_owner", "rfx_dev_bucket_wide_records_by_owner"), k)


def test_entries_refuse_k_beyond_their_own_bound(rfx, scratch):
    """k = 129 is a k of the counter (the sort path takes it: RFX_OK from the host entries and rfx_dev_count_reads_w), but
    beyond the bucketed entries rfx_dev_count_reads_ragged_w, rfx_dev_count_wide_elems and rfx_dev_order_kmers_w (k <= 127);
    the two-word record and owner-bucket entries end at k = 63 and refuse k = 65"""
    s = scratch
    s.refill()
    e = entries(rfx, s, 129)
    for nm in ("rfx_extract_canon_w", "rfx_count_filter_w", "rfx_dev_count_reads_w"):
        assert e[nm]() == OK, nm
    refused(rfx, s, ("rfx_dev_count_reads_ragged_w", "rfx_dev_count_wide_elems", "rfx_dev_order_kmers_w"), 129)
    refused(rfx, s, ("rfx_dev_count_wide_records", "rfx_dev_bucket_wide_by_owner", "rfx_dev_bucket_wide_records_by_owner"), 65)
    refused(rfx, s, ("rfx_dev_count_reads", "rfx_dev_count_reads_ragged", "rfx_dev_combine_reads", "rfx_dev_bucket_by_owner",
                     "rfx_dev_bucket_records_by_owner", "rfx_extract_canon"), 33)


def assemble_reads_raw(rfx, prm):
    """rfx_assemble_reads through ctypes on 50 reads of 200 bases -> (status, whether every output is as it was)"""
    rng = np.random.default_rng(1)
    bases, off = reads_of(["".join(rng.choice(list("ACGT"), size=200)) for _ in range(50)])
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    text, trace = np.full(1 << 16, FILL, np.uint8), np.empty(64, np.int64)
    trace.view(np.uint8).fill(FILL)
    ln, nc, ntr, kept = i64(-77), i64(-77), i64(-77), i64(-77)
    st = rfx.L.rfx_assemble_reads(rfx.ctx, hp(bases), hp(off), i64(len(off) - 1), C.byref(prm), hp(text), i64(len(text)), C.byref(ln), C.byref(nc),
                                  hp(trace), i64(len(trace)), C.byref(ntr), C.byref(kept))
    same = (text == FILL).all() and (trace.view(np.uint8) == FILL).all() and (ln.value, nc.value, ntr.value, kept.value) == (-77,) * 4
    return st, bool(same)


@pytest.mark.parametrize("k", [126, 127, 128, 32, 64, 96, 2])
def test_assemble_reads_refuses(rfx, k):
    """rfx_assemble_reads takes k = 3..31 and 33..125 (not 64 or 96): the driver's keys end at four words.  The text, the
    trace, *out_len, *out_contigs, *n_trace and *out_kept are left alone; the Python wrapper raises RfxError"""
    import reflexiv_amd
    prm = reflexiv_amd.default_params(k=k, min_cov=1, partitions=2)
    assert assemble_reads_raw(rfx, prm) == (E_ARG, True)
    with pytest.raises(reflexiv_amd.RfxError) as ei:
        rfx.assemble_reads(READS, READ_OFF, prm)
    assert ei.value.status == E_ARG


CLIPPED_W = ("rfx_extract_canon_w", "rfx_dev_count_reads_w", "rfx_dev_count_reads_ragged_w", "rfx_dev_bucket_wide_by_owner",
             "rfx_dev_bucket_wide_records_by_owner")
CLIPPED = ("rfx_extract_canon", "rfx_dev_count_reads", "rfx_dev_count_reads_ragged", "rfx_dev_combine_reads", "rfx_dev_bucket_by_owner",
           "rfx_dev_bucket_records_by_owner")


@pytest.mark.parametrize("fc,ec", [(-1, 0), (0, -1), (-3, -5)])
def test_negative_clips_are_refused(rfx, scratch, fc, ec):
    """a negative front or end clip: RFX_E_ARG from every entry that takes clips, k <= 31 and beyond (only those are called),
    with every buffer, *out_n, *out_distinct and *out_instances as they were; rfx_assemble_reads likewise"""
    import reflexiv_amd
    refused(rfx, scratch, CLIPPED, 31, front_clip=fc, end_clip=ec)
    for k in (63, 95, 129):
        names = [nm for nm in CLIPPED_W if (k < 64 or "bucket" not in nm) and (k < 128 or "ragged" not in nm)]
        refused(rfx, scratch, names, k, front_clip=fc, end_clip=ec)
    for k in (31, 63):
        assert assemble_reads_raw(rfx, reflexiv_amd.default_params(k=k, min_cov=1, partitions=2, front_clip=fc, end_clip=ec)) == (E_ARG, True)


def test_reads_wider_than_their_words_are_refused(rfx, scratch):
    """words_per_read * 32 < read_len (6 words for 200 bases): RFX_E_ARG from every entry that takes packed reads, with
    nothing written"""
    refused(rfx, scratch, [nm for nm in CLIPPED if nm != "rfx_extract_canon"], 31, wpr=6)
    for k in (63, 95, 129):
        names = [nm for nm in CLIPPED_W if nm != "rfx_extract_canon_w" and (k < 64 or "bucket" not in nm) and (k < 128 or "ragged" not in nm)]
        refused(rfx, scratch, names, k, wpr=6)
