"""Level 1's one sweep (k_sk_onesweep) where the order of its memory waits can go wrong: a bin that one round floods (the
drain moves up ONE extent and never claims; more than the two extents in hand take makes the sweep void and the two-pass
form runs), inputs whose last tile has 1, T - 1, T or T + 1 segments (the segment's words are loaded without a branch: a lane
past the last segment reads the last segment's), and the same input twice.

Every case forces the sweep (RFX_SK_ONESWEEP=2) and compares the counts key for key with the oracle at min_cov 1.
count_timing()["stat_records"] is the number of records a sweep that STOOD wrote (0: the two-pass form ran), and
count_timing()["stat_l1_void_rounds"] says that a round raised the flag -- not a region that ran out.

Shapes: PE150 at k = 31 is 120 windows = 4 segments of 32 windows a read, so a tile of 512 segments is 128 reads; the
16-window forms (k = 63: 88 windows, 6 segments a read; RFX_LEVEL_BITS=10,1: 8 segments a read) have tiles of 1024 segments.
The flooded block starts at read 512, which is a tile's first read in all three.  16,384 reads are 128 tiles of 512 segments
and 64 sampled tiles, so every tile is sampled; a bin then holds 4 records a tile on average (16 records a read, 512 bins)
and the copies add B x c / 128 to the busiest (c: the read's records in that bin), which stays under 16: extents of 64.

Run on the MI355X box:  python -m pytest tests/test_gpu_l1sweep_waits.py -m gpu -q
"""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

L = 150
N_FLOOD = 16_384
FLOOD_AT = 512                 # first read of a tile in every form (see above)
FLOODS = [40, 70, 100, 128]
EDGE_COUNTS = [1, 127, 128, 129, 8_191, 8_192, 8_193]


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


@pytest.fixture(scope="module")
def pool():
    """16,384 random PE150 reads off a 60 kbp genome as an ASCII matrix [n, 150], made once and never changed"""
    G = 60_000
    g = O.synth_genome(41, G)
    bases, off = O.synth_reads(41, g, G, 0, N_FLOOD, L)
    assert len(bases) == N_FLOOD * L and np.array_equal(np.diff(off), np.full(N_FLOOD, L))
    m = np.ascontiguousarray(bases, np.uint8).reshape(N_FLOOD, L)
    m.setflags(write=False)
    return m


def as_arrays(rows, lens):
    """rows [n, >= max(lens)] ASCII, lens [n] -> (bases, off) with read i = rows[i, :lens[i]]"""
    lens = np.asarray(lens, np.int64)
    keep = np.arange(rows.shape[1])[None, :] < lens[:, None]
    bases = np.ascontiguousarray(rows[keep])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return bases, off


def oracle_counts(bases, off, k):
    """-> (keys [m, W] uint64, counts int64[m]) at min_cov 1"""
    if k > 32:
        wk, wc, _ = O.count_filter_w(O.extract_canon_w(bases, off, k), k, 1)
        return np.asarray(wk).reshape(len(wc), -1), np.asarray(wc).astype(np.int64)
    wk, wc, _ = O.count_filter(O.extract_canon(bases, off, k), 1)
    return np.asarray(wk).reshape(-1, 1), np.asarray(wc).astype(np.int64)


def device_counts(rfx, torch, bases, off, k, bits, ragged, monkeypatch):
    """-> (keys [m, W] uint64, counts int64[m], instances, records the sweep wrote, void rounds)"""
    monkeypatch.setenv("RFX_SK_ONESWEEP", "2")
    monkeypatch.setenv("RFX_LEVEL_BITS", bits)
    n = len(off) - 1
    maxlen = int(np.diff(off).max())
    wpr = (maxlen + 31) // 32
    db = torch.from_numpy(bases.copy()).cuda()
    do = torch.from_numpy(off.copy()).cuda()
    dw = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    dl = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rfx.encode_reads_dev(db.data_ptr(), do.data_ptr(), n, wpr, dw.data_ptr(), dl.data_ptr())
    rfx.sync()
    wide = k > 32
    W = 2 if wide else 1
    cap = max(1, (maxlen - k + 1) * n) + 1
    dk = torch.empty(W * cap, dtype=torch.int64, device="cuda")
    dc = torch.empty(cap, dtype=torch.int64 if wide else torch.int32, device="cuda")
    torch.cuda.synchronize()
    if wide:
        assert not ragged
        m, nd, inst = rfx.count_reads_w_dev(dw.data_ptr(), n, wpr, maxlen, k, dk.data_ptr(), dc.data_ptr(), cap, 1)
    elif ragged:
        m, nd, inst = rfx.count_reads_ragged_dev(dw.data_ptr(), dl.data_ptr(), n, wpr, maxlen, k, dk.data_ptr(), dc.data_ptr(), cap, 1)
    else:
        m, nd, inst = rfx.count_reads_dev(dw.data_ptr(), n, wpr, maxlen, k, dk.data_ptr(), dc.data_ptr(), cap, 1)
    t = rfx.count_timing()
    keys = dk[:W * m].cpu().numpy().view(np.uint64).reshape(m, W)
    return (keys, dc[:m].cpu().numpy().astype(np.int64), inst, t.get("stat_records", (0.0, 0))[1],
            t.get("stat_l1_void_rounds", (0.0, 0))[1])


def same(got, want):
    return got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def flooded(pool, B):
    rows = pool.copy()
    rows[FLOOD_AT:FLOOD_AT + B] = rows[FLOOD_AT]
    return as_arrays(rows, np.full(len(rows), L))


@pytest.mark.parametrize("k,bits", [(31, "9,1"), (63, "9,1"), (31, "10,1")])
def test_one_bin_flooded_in_one_round(rfx, torch_mod, pool, k, bits, monkeypatch):
    """B of the 128 reads of one tile are copies of one read, B = 40, 70, 100, 128.  Every B gives the oracle's counts.  At 128
    every bin the read touches receives 128 records or more in one round: two whole extents of 64, which fit only behind an
    extent that is exactly empty and with nothing else for the bin in that tile -- so a round raises the flag
    (stat_l1_void_rounds), the sweep is void (stat_records 0) and the two-pass form counts.  Which smaller B stand depends on
    how far the bin's extent was filled when the tile came (the tiles are handed out by a counter): printed, not asserted.
    On the MI355X, in all three forms: B = 40 stood; 70, 100 and 128 were void (one void round each) and fell back."""
    stood = {}
    for B in FLOODS:
        bases, off = flooded(pool, B)
        got = device_counts(rfx, torch_mod, bases, off, k, bits, False, monkeypatch)
        stood[B] = (got[3] > 0, got[4])
        assert got[2] == (L - k + 1) * N_FLOOD
        assert same(got, oracle_counts(bases, off, k)), (k, bits, B)
        assert not (got[3] > 0 and got[4] > 0), (B, got[3], got[4])                  # a sweep that stood raised no flag
    print(f"k = {k}, bits {bits}: (the sweep stood, void rounds) by B: {stood}")
    assert stood[128] == (False, 1), stood


@pytest.fixture(scope="module")
def edge_reference(pool):
    """the oracle's counts of the tile-edge cases, made once per (n, read length, ragged)"""
    cache = {}

    def get(n, length, ragged):
        key = (n, length, ragged)
        if key not in cache:
            lens = np.full(n, length)
            if ragged:                                   # 31 (no window) .. length, the first read full: the longest stays `length`
                lens = np.random.default_rng(n + length).integers(31, length + 1, size=n)
                lens[0] = length
            bases, off = as_arrays(pool[:n], lens)
            cache[key] = (bases, off, oracle_counts(bases, off, 31), int(np.where(lens - 31 <= 1, 0, lens - 30).sum()))
        return cache[key]
    return get


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("length", [L, L + 1 - 31, 33], ids=["L150", "L120", "L33"])
@pytest.mark.parametrize("n", EDGE_COUNTS)
def test_tile_edges(rfx, torch_mod, pool, edge_reference, n, length, ragged, monkeypatch):
    """1 .. 8,193 reads of 150 bases (4 segments: tiles of 128 reads), of 151 - k = 120 bases (90 windows, 3 segments: reads
    straddle the tiles) and of k + 2 = 33 bases (the shortest read that emits at k <= 31: 3 windows, one segment, tiles of 512
    reads, so 8,192 reads are 16 full tiles and 8,193 leave a tile of one segment), of one length and of lengths 31 .. L:
    the last tile's lanes past the end and the reads without a window bring nothing, and no load leaves the read store."""
    assert n <= len(pool)
    bases, off, want, inst = edge_reference(n, length, ragged)
    got = device_counts(rfx, torch_mod, bases, off, 31, "9,1", ragged, monkeypatch)
    assert got[2] == inst
    assert same(got, want)
    assert got[3] > 0 and got[4] == 0, got[3:]


def test_the_same_input_twice(rfx, torch_mod, pool, monkeypatch):
    """the flooded set of B = 70 twice in one process: which workgroup takes which tile differs from run to run, the counts
    may not"""
    bases, off = flooded(pool, 70)
    a = device_counts(rfx, torch_mod, bases, off, 31, "9,1", False, monkeypatch)
    b = device_counts(rfx, torch_mod, bases, off, 31, "9,1", False, monkeypatch)
    assert same(a, b) and a[2] == b[2]
    assert same(a, oracle_counts(bases, off, 31))
