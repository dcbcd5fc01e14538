"""Level 1's one sweep cuts super-k-mer runs by the sequence, not at the edges of a thread's 32 windows (seg_runs, SEG = 32):
the tail run of a full segment and the head run of the same read's next segment are one record when their minimiser keys
are equal, up to 16 windows from where the run started.

The records of the sweep do not leave the library (rfx_dev_bucket_records_by_owner runs the two-pass, 16-window form; the
sweep's owner form is only reached inside rfx_dev_sharded_count), so the cut is checked from outside in two ways: the
COUNTS must be the oracle's -- every window in exactly one record, every base right, the ones from the neighbour lane
included -- and the NUMBER of records the sweep wrote (count_timing()["stat_records"]) must be what a numpy model of the
merged cut rule says, wave edges included: one record too many or too few anywhere shows.

Run on the MI355X box:  python -m pytest tests/test_gpu_run_merge.py -m gpu -q
"""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

SK_M = 13
SEG = 32
CAP = 16
WAVE = 64


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


def model_records(bases, off, k, max_len):
    """-> (records without merging, records with merging) of the 32-window cut, for reads given as ASCII.

    As the device does it: a base is A0 C1 G2, anything else 3, a short read is padded with A and has len - k + 1 windows
    (none when len <= k + 1); an m-mer's key is
    umul24(canonical 13-mer, 0x9E3779) + canonical 13-mer in 32 bits; a window's minimiser key is the smallest key of its
    k - 12 m-mers; a run is a stretch of windows with equal keys inside one segment of 32 windows, cut 16 windows after
    its start.  Merged: the tail of a full segment and the head of the same read's next segment (lanes g, g + 1 with
    g = read * segments + segment, both in one wave of 64) with equal keys are one run of min(16, t + b) windows -- one
    record less when t + b <= 16, the same number otherwise."""
    n = len(off) - 1
    lens = np.diff(off).astype(np.int64)
    lut = np.full(256, 3, np.uint32)
    lut[ord("A")], lut[ord("C")], lut[ord("G")] = 0, 1, 2
    codes = np.zeros((n, max_len), np.uint32)
    col = np.arange(max_len)[None, :]
    inside = col < lens[:, None]
    codes[inside] = lut[bases]                     # (reads are stored back to back, in order)
    nm, nk, W = max_len - SK_M + 1, max_len - k + 1, k - SK_M + 1
    f = np.zeros((n, nm), np.uint32)
    r = np.zeros((n, nm), np.uint32)
    for j in range(SK_M):
        f = (f << np.uint32(2)) | codes[:, j:j + nm]
        r |= (np.uint32(3) - codes[:, j:j + nm]) << np.uint32(2 * j)
    canon = np.minimum(f, r).astype(np.uint64)
    key = ((canon & np.uint64(0xFFFFFF)) * np.uint64(0x9E3779) + canon) & np.uint64(0xFFFFFFFF)
    wm = np.lib.stride_tricks.sliding_window_view(key, W, axis=1).min(axis=2)
    assert wm.shape == (n, nk)
    segs = (nk + SEG - 1) // SEG
    nk_r = np.where(lens - k <= 1, 0, np.clip(lens - k + 1, 0, nk))      # (the reference's skip rule: a read of k or k + 1 bases emits nothing)
    wmp = np.zeros((n, segs * SEG), np.uint64)
    wmp[:, :nk] = wm
    valid = np.arange(segs * SEG)[None, :] < nk_r[:, None]
    start = np.ones((n, segs * SEG), bool)
    start[:, 1:] = wmp[:, 1:] != wmp[:, :-1]
    start[:, ::SEG] = True
    start &= valid
    S, V, K = start.reshape(n, segs, SEG), valid.reshape(n, segs, SEG), wmp.reshape(n, segs, SEG)
    run = np.zeros((n, segs), np.int64)
    for i in range(SEG):                           # no run longer than 16 windows
        S[:, :, i] |= V[:, :, i] & (run == CAP)
        run = np.where(S[:, :, i], 1, run + 1)
    plain = int(S.sum())
    v = V.sum(axis=2)
    later = S.copy()
    later[:, :, 0] = False
    b = np.where(later.any(axis=2), later.argmax(axis=2), v)              # head: windows of the first run
    t = v - (SEG - 1 - S[:, :, ::-1].argmax(axis=2))                      # tail: windows of the last run (full segments)
    g = np.arange(n)[:, None] * segs + np.arange(segs)[None, :]
    edge = (v[:, :-1] == SEG) & (v[:, 1:] > 0) & (K[:, :-1, SEG - 1] == K[:, 1:, 0]) & (g[:, :-1] % WAVE != WAVE - 1)
    gone = edge & (t[:, :-1] + b[:, 1:] <= CAP)
    return plain, plain - int(gone.sum())


def genome_reads(seed, n_reads, L, G=30_000):
    g = O.synth_genome(seed, G)
    return O.synth_reads(seed, g, G, 0, n_reads, L)


def low_complexity(L, n_a, n_ac, n_one, n_t, n_rand, n_n, seed):
    rng = np.random.default_rng(seed)
    one = "".join(rng.choice(list("ACGT"), size=L))
    reads = ["A" * L] * n_a + ["AC" * (L // 2)] * n_ac + [one] * n_one + ["T" * L] * n_t + \
            ["".join(rng.choice(list("ACGT"), size=L)) for _ in range(n_rand)] + ["N" * L] * n_n
    rng.shuffle(reads)
    return reads


def as_arrays(reads):
    bases = np.frombuffer("".join(reads).encode(), np.uint8)
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.int64)
    return bases, off


def make_case(name):
    """-> (bases, off, k, longest read, ragged, the sweep must run)"""
    if name.startswith("k"):                      # "k31-L150": uniform reads off a 30 kbp genome
        k, L = (int(x[1:]) for x in name.split("-"))
        bases, off = genome_reads(100 + k + L, 40_000 if L < 100 else 30_000, L)
        return bases, off, k, L, False, True
    if name == "skew":                            # the mix of test_count_survives_extreme_skew: whichever form of level 1 takes it
        bases, off = as_arrays(low_complexity(150, 12000, 6000, 5000, 3000, 2000, 10, 31))
        return bases, off, 31, 150, False, False
    if name == "skew-diluted":
        # the same kinds of reads among genome reads, few enough of each that the sampled histogram lets the sweep run (a
        # tile of 512 segments must not bring one bucket more than 64 records): poly-A / poly-T / N reads are ONE key from end
        # to end, so every edge merges or is capped -- t + b > 16 and chains of capped runs over all segments of a read
        b0, o0 = genome_reads(7, 28_000, 150)
        reads = [bytes(b0[o0[i]:o0[i + 1]]).decode() for i in range(28_000)] + low_complexity(150, 500, 500, 500, 250, 0, 10, 5)
        np.random.default_rng(9).shuffle(reads)
        bases, off = as_arrays(reads)
        return bases, off, 31, 150, False, True
    assert name == "ragged"                       # lengths 31..150: empty and partial segments beside full ones
    rng = np.random.default_rng(77)
    b0, o0 = genome_reads(8, 30_000, 150)
    lens = rng.integers(31, 151, size=30_000)
    lens[:8] = 150
    reads = [bytes(b0[o0[i]:o0[i] + lens[i]]).decode() for i in range(30_000)]
    bases, off = as_arrays(reads)
    return bases, off, 31, 150, True, True


CASES = ["k31-L150",      # 4 segments: lanes aligned to reads, nothing straddles a wave
         "k21-L150",      # 130 windows, 5 segments: reads straddle waves, the last segment has 2 windows
         "k31-L62",       # exactly 32 windows: one segment, nothing to merge
         "k31-L63",       # a second segment of one window
         "k31-L94",       # two full segments
         "k31-L95",       # ... and a third of one window
         "skew", "skew-diluted", "ragged"]


@pytest.mark.parametrize("name", CASES)
def test_merged_runs_count_like_the_oracle(rfx, torch_mod, name, monkeypatch):
    """counts at min_cov 1 and 2 equal the oracle's with level 1 forced through the one sweep, and the sweep wrote as many
    records as the model of the merged cut says -- three calls, the same every time"""
    torch = torch_mod
    monkeypatch.setenv("RFX_SK_ONESWEEP", "2")
    monkeypatch.setenv("RFX_LEVEL_BITS", "9,1")
    bases, off, k, L, ragged, must_sweep = make_case(name)
    n = len(off) - 1
    wpr = (L + 31) // 32
    km = O.extract_canon(bases, off, k)
    plain, merged = model_records(bases, off, k, L)
    nk = L - k + 1
    print(f"{name}: {n} reads, {len(km)} windows, model: {plain} records cut at every segment edge, {merged} merged")
    assert merged <= plain and (merged < plain) == (nk > SEG)
    db = torch.from_numpy(bases.copy()).cuda(); do = torch.from_numpy(off).cuda()
    dw = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    dl = torch.empty(n, dtype=torch.int32, device="cuda")
    dk = torch.empty(len(km) + 1, dtype=torch.int64, device="cuda"); dc = torch.empty(len(km) + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rfx.encode_reads_dev(db.data_ptr(), do.data_ptr(), n, wpr, dw.data_ptr(), dl.data_ptr())
    for min_cov in (1, 2, 2):
        if ragged:
            m, nd, inst = rfx.count_reads_ragged_dev(dw.data_ptr(), dl.data_ptr(), n, wpr, L, k, dk.data_ptr(), dc.data_ptr(),
                                                     len(km) + 1, min_cov)
        else:
            m, nd, inst = rfx.count_reads_dev(dw.data_ptr(), n, wpr, L, k, dk.data_ptr(), dc.data_ptr(), len(km) + 1, min_cov)
        wk, wc, wd = O.count_filter(km, min_cov)
        assert inst == len(km) and nd == wd and m == len(wk)
        assert np.array_equal(dk[:m].cpu().numpy().view(np.uint64), wk) and np.array_equal(dc[:m].cpu().numpy(), wc)
        wrote = rfx.count_timing().get("stat_records", (0.0, 0))[1]
        print(f"  min_cov {min_cov}: the sweep wrote {wrote} records")
        if must_sweep:
            assert wrote == merged, (wrote, merged, plain)
        else:
            assert wrote in (0, merged), (wrote, merged, plain)          # (0: the two-pass form took the set)
