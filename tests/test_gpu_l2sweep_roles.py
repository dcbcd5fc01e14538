"""The last radix level in one sweep (k_rec_l2sweep) at the smallest shapes where its tile loop, its rings and its spill path can
go wrong: parents whose sizes sit on the edges of the kernel's tile, parents that lie in ONE child (every tile overruns a ring),
1024 children, and the same input twice.  The records come from random reads (bucket_*_records_by_owner_dev), are selected on
the host by the digits of their header word -- so parents have exact sizes -- and are counted with count_records_dev /
count_wide_records_dev under RFX_LEVEL_BITS.  References: the exact form (RFX_L2_ONESWEEP=0), a host count of the k-mers the
records expand to (numpy, k = 31), and the oracle where whole reads are counted.  `stat_l2_sweeps` tells a sweep that ran and
stood from a silent fall-back to the exact form.

The plan tries a sweep only when the regions -- sized from a 1/16 sample with a floor of 608 records a child -- fit into
2 n + 640 records a child; at 256 children and 135,209 records (and at 16,384 children and 4.5 M) they miss that by 3 % and
by 0.7 %, so those cases run at RFX_L2_SQUEEZE=85: regions of 85 %, still about three times what the children hold."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

T = 4096                       # records of one tile of k_rec_l2sweep (WCT x WC_PER; the 16- and the 32-byte records alike)
EDGE_SIZES = [0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 5] + [3 * T + 5] * 7      # the 16 parents of "4,4"
FIT = "85"                     # see the module docstring


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


def make_reads_dev(rfx, torch, seed, genome_len, n_reads, read_len):
    wpr = (read_len + 31) // 32
    dg = torch.empty((genome_len + 31) // 32, dtype=torch.int64, device="cuda")
    dw = torch.empty(n_reads * wpr, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rfx.synth_genome_dev(seed, genome_len, dg.data_ptr())
    rfx.synth_reads_dev(seed, dg.data_ptr(), genome_len, 0, n_reads, read_len, wpr, dw.data_ptr())
    rfx.sync()
    return dg, dw, wpr


def records_of_reads(rfx, torch, k, seed, G, n_reads, L=150):
    """-> uint64[n, 2] (k <= 31) or uint64[n, 4] (k = 33..63): the super-k-mer records of the reads"""
    dg, dw, wpr = make_reads_dev(rfx, torch, seed, G, n_reads, L)
    wide = k > 32
    fn = rfx.bucket_wide_records_by_owner_dev if wide else rfx.bucket_records_by_owner_dev
    width = 4 if wide else 2
    doff = torch.empty(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    need, _ = fn(dw.data_ptr(), n_reads, wpr, L, k, 1, 0, 0, doff.data_ptr())
    out = torch.empty(width * need, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nrec, h = fn(dw.data_ptr(), n_reads, wpr, L, k, 1, out.data_ptr(), need, doff.data_ptr())
    assert nrec == need and h is not None
    return out.cpu().numpy().view(np.uint64).reshape(nrec, width)


@pytest.fixture(scope="module")
def pool(rfx, torch_mod):
    """records of 40,000 random reads per k, made once: what the cases select from"""
    cache = {}

    def get(k):
        if k not in cache:
            cache[k] = records_of_reads(rfx, torch_mod, k, 11 + k, 30_000, 40_000)
        return cache[k]
    return get


def header(recs):
    return (recs[:, -1] & np.uint64(0xFFFFFFFF)).astype(np.uint32)      # (w1 of a 16-byte record, hd of a 32-byte one)


def windows(recs):
    return ((recs[:, -1] >> np.uint64(32)) & np.uint64(15)).astype(np.int64) + 1


def select_parents(recs, sizes, seed=5):
    """sizes[p] records whose first 4-bit digit is p, in a fixed random order"""
    top = header(recs) >> np.uint32(28)
    parts = []
    for p, sz in enumerate(sizes):
        idx = np.flatnonzero(top == p)
        assert len(idx) >= sz, (p, len(idx), sz)
        parts.append(idx[:sz])
    idx = np.concatenate(parts)
    np.random.default_rng(seed).shuffle(idx)
    return np.ascontiguousarray(recs[idx])


def count_records(rfx, torch, recs, k, bits, sweep, squeeze, monkeypatch, min_cov=2):
    """-> (keys uint64[m, W], counts int64[m], {stat: n}) of the records under RFX_LEVEL_BITS = bits"""
    monkeypatch.setenv("RFX_LEVEL_BITS", bits)
    monkeypatch.setenv("RFX_L2_ONESWEEP", sweep)
    monkeypatch.setenv("RFX_L2_SQUEEZE", squeeze)
    wide = k > 32
    W = 2 if wide else 1
    n = len(recs)
    n_inst = int(windows(recs).sum())
    cap = n_inst // 2 + 1024
    d = torch.from_numpy(recs.view(np.int64).reshape(-1).copy()).cuda()
    dk = torch.empty(W * cap, dtype=torch.int64, device="cuda")
    dc = torch.empty(cap, dtype=torch.int64 if wide else torch.int32, device="cuda")
    torch.cuda.synchronize()
    if wide:
        m, _ = rfx.count_wide_records_dev(d.data_ptr(), n, 0, k, dk.data_ptr(), dc.data_ptr(), cap, min_cov)
    else:
        m, _ = rfx.count_records_dev(d.data_ptr(), n, n_inst, k, dk.data_ptr(), dc.data_ptr(), cap, min_cov)
    t = rfx.count_timing()
    stats = {s: t.get("stat_l2_" + s, (0, 0))[1] for s in ("sweeps", "spilled", "void")}
    return dk[:W * m].cpu().numpy().view(np.uint64).reshape(m, W), dc[:m].cpu().numpy().astype(np.int64), stats


def host_count_31(recs, min_cov=2):
    """the canonical 31-mers of the records' windows (LeafElem<1>::for_each_kmer restated), counted and filtered -> sorted keys, counts"""
    k = 31
    w0, w1 = recs[:, 0].copy(), recs[:, 1].copy()
    n = windows(recs)
    u = np.uint64
    fwd = w0 >> u(2)
    rest = (w0 << u(62)) | (w1 >> u(2))
    mask = u((1 << 62) - 1)
    rc = np.zeros_like(fwd)
    for j in range(k):                                           # base j from the end goes to place j from the front, complemented
        rc |= (((fwd >> u(2 * j)) & u(3)) ^ u(3)) << u(2 * (k - 1 - j))
    out = []
    for i in range(16):
        out.append(np.minimum(fwd, rc)[n > i])
        b = rest >> u(62)
        rest = rest << u(2)
        fwd = ((fwd << u(2)) | b) & mask
        rc = (rc >> u(2)) | ((b ^ u(3)) << u(60))
    keys, counts = np.unique(np.concatenate(out), return_counts=True)
    keep = counts >= min_cov
    return keys[keep].reshape(-1, 1), counts[keep].astype(np.int64)


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def edge_case(pool):
    """case 1's input and its host count, per k, made once"""
    cache = {}

    def get(k):
        if k not in cache:
            recs = select_parents(pool(k), EDGE_SIZES)
            cache[k] = (recs, host_count_31(recs) if k == 31 else None)
        return cache[k]
    return get


@pytest.mark.parametrize("k", [31, 63])
def test_parents_on_the_tile_edges(rfx, torch_mod, edge_case, k, monkeypatch):
    """16 parents x 16 children (RFX_LEVEL_BITS=4,4), the parents of 0, 1, T - 1, T, T + 1, 2T - 1, 2T, 2T + 1 and 3T + 5 records
    (T = 4096, the kernel's tile; the largest under 1.5 x mean + 4096, or the plan would not try the sweep): the tile loop's
    first, last, full, one-record and empty tiles.  Survivors of the sweep = those of the exact form = the host count."""
    recs, want = edge_case(k)
    assert len(recs) == sum(EDGE_SIZES) >= 65536 and max(EDGE_SIZES) < 1.5 * len(recs) / 16 + 4096
    exact = count_records(rfx, torch_mod, recs, k, "4,4", "0", FIT, monkeypatch)
    sweep = count_records(rfx, torch_mod, recs, k, "4,4", "1", FIT, monkeypatch)
    assert exact[2]["sweeps"] == 0
    assert sweep[2]["sweeps"] == 1 and sweep[2]["void"] == 0, sweep[2]
    assert len(exact[0]) > 10_000
    assert same(sweep, exact)
    if want is not None:
        assert same(sweep, want)


@pytest.mark.parametrize("k", [31, 63])
def test_parents_that_lie_in_one_child(rfx, torch_mod, pool, k, monkeypatch):
    """every parent is 20,000 copies of one record: one child takes all of it, every tile overruns that child's ring (what the
    ring does not take is stored directly, beyond the child's region it goes to the spill list).  The sample sees 3 x 512 of
    them, the region is 28,856 records: at RFX_L2_SQUEEZE=100 the sweep stands with nothing spilled, at 60 (17,312) 16 x 2,688
    records spill and are moved with their children, at 30 (8,656) more spill than the list takes and the exact form runs."""
    src = pool(k)
    top = header(src) >> np.uint32(28)
    one = np.stack([src[np.flatnonzero(top == p)[0]] for p in range(16)])
    recs = np.ascontiguousarray(np.repeat(one, 20_000, axis=0))
    np.random.default_rng(9).shuffle(recs, axis=0)
    exact = count_records(rfx, torch_mod, recs, k, "4,4", "0", "100", monkeypatch)
    assert exact[2]["sweeps"] == 0 and 1 <= len(exact[0]) <= 16 * 16 and exact[1].min() >= 20_000
    if k == 31:
        assert same(exact, host_count_31(recs))
    for squeeze, want in (("100", {"sweeps": 1, "spilled": 0, "void": 0}), ("60", {"sweeps": 1, "spilled": 16 * 2688, "void": 0}),
                          ("30", {"sweeps": 0, "spilled": 0, "void": 1})):
        got = count_records(rfx, torch_mod, recs, k, "4,4", "1", squeeze, monkeypatch)
        assert got[2] == want, (squeeze, got[2])
        assert same(got, exact), squeeze


def test_1024_children(rfx, torch_mod, monkeypatch):
    """RFX_LEVEL_BITS=4,10 at k = 31: the 8-slot rings of 1024 children (the sweep's longest drain), tried from 16 x 1024 x 256
    records on -- the records of 280,000 whole reads, so the oracle counts the reads."""
    seed, G, n_reads, L, k = 23, 200_000, 280_000, 150, 31
    recs = records_of_reads(rfx, torch_mod, k, seed, G, n_reads, L)
    assert len(recs) >= 16 * 1024 * 256 and int(windows(recs).sum()) == (L - k + 1) * n_reads
    sweep = count_records(rfx, torch_mod, recs, k, "4,10", "1", FIT, monkeypatch)
    exact = count_records(rfx, torch_mod, recs, k, "4,10", "0", FIT, monkeypatch)
    assert sweep[2]["sweeps"] == 1 and sweep[2]["void"] == 0 and exact[2]["sweeps"] == 0, (sweep[2], exact[2])
    assert same(sweep, exact)
    g = O.synth_genome(seed, G)
    bases, off = O.synth_reads(seed, g, G, 0, n_reads, L)
    O.set_threads(min(16, O.host_cores()))
    try:
        wk, wc, _, ni = O.count_reads_omp(bases, off, k, 2, cap=8_000_000)
    finally:
        O.set_threads(1)
    order = np.argsort(wk)
    assert ni == (L - k + 1) * n_reads
    assert same(sweep, (wk[order].reshape(-1, 1), wc[order].astype(np.int64)))


def test_the_same_input_twice(rfx, torch_mod, edge_case, monkeypatch):
    """case 1 twice in one process: the order inside a child may differ from run to run, the survivors may not"""
    recs, want = edge_case(31)
    a = count_records(rfx, torch_mod, recs, 31, "4,4", "1", FIT, monkeypatch)
    b = count_records(rfx, torch_mod, recs, 31, "4,4", "1", FIT, monkeypatch)
    assert a[2]["sweeps"] == 1 and b[2]["sweeps"] == 1
    assert same(a, b) and same(a, want)
