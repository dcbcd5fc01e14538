"""Three- and four-word k-mers (k = 65..127, not 96) on the device: the W-word element path at W = 3, 4 (W = 2:
tests/test_gpu_count_w2_elems.py;
level 1 straight from the packed reads, record levels on a hash of all words, LDS-table leaves with W key planes).
rfx_dev_count_reads_w / rfx_dev_count_reads_ragged_w against the oracle's k > 31 counter, rfx_assemble_reads against the
reference's two-step route (`counter -kmer K`, then `run -kmerc ... -kmer K`) and the reference-made k = 95 vector, and the
CLI's --resident twins.  Bit-exact (integer work)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import test_reference_vectors as T
from tests.test_gpu_ragged_w import host_bin, upload, write_fq

pytestmark = pytest.mark.gpu

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "n": "n", "a": "t", "c": "g", "g": "c", "t": "a"}


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


def ragged_reads_w(seed, k, n_reads=3000, genome_len=20_000, err=0.0):
    """seeded reads of the edge lengths around k, 96 / 128 and 251, and random lengths up to 251, with N, lower case and
    (err > 0) substitutions"""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), size=genome_len))
    edge = [0, 1, k - 1, k, k + 1, 96, 97, 128, 129, 150, 251]
    reads = []
    for i in range(n_reads):
        L = edge[i % len(edge)] if i < 4 * len(edge) else int(rng.integers(k - 3, 252))
        p = int(rng.integers(0, genome_len - L))
        s = list(genome[p:p + L])
        if err:
            for j in np.nonzero(rng.random(L) < err)[0]:
                s[j] = "ACGT"[("ACGT".index(s[j]) + int(rng.integers(1, 4))) % 4]
        if L and rng.random() < 0.05:
            s[int(rng.integers(0, L))] = "N"
        if L and rng.random() < 0.05:
            j = int(rng.integers(0, L))
            s[j] = s[j].lower()
        if rng.random() < 0.5:
            s = [COMP[c] for c in reversed(s)]
        reads.append("".join(s))
    return reads_of(reads)


def count_ragged(rfx, torch, dw, dl, n, wpr, maxlen, k, cap, min_cov=2, max_cov=10_000_000, clips=(0, 0)):
    W = k // 32 + 1
    dk = torch.empty(max(1, cap) * W, dtype=torch.int64, device="cuda")
    dc = torch.empty(max(1, cap), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m, nd, inst = rfx.count_reads_ragged_w_dev(dw.data_ptr(), dl.data_ptr(), n, wpr, maxlen, k, dk.data_ptr(), dc.data_ptr(),
                                               max(1, cap), min_cov, max_cov, front_clip=clips[0], end_clip=clips[1])
    return m, nd, inst, dk[:W * m].cpu().numpy().view(np.uint64).reshape(m, W), dc[:m].cpu().numpy()


def check_ragged(rfx, torch, bases, off, k, min_covs=(1, 2), max_cov=10_000_000, clips=(0, 0)):
    dw, dl, n, wpr, maxlen = upload(rfx, torch, bases, off)
    km = O.extract_canon_w(bases, off, k, *clips)
    for min_cov in min_covs:
        m, nd, inst, keys, counts = count_ragged(rfx, torch, dw, dl, n, wpr, maxlen, k, len(km), min_cov, max_cov, clips)
        wk, wc, wd = O.count_filter_w(km, k, min_cov, max_cov)
        assert (inst, nd, m) == (len(km), wd, len(wk)), (k, min_cov, clips)
        assert np.array_equal(keys, wk) and np.array_equal(counts, wc), (k, min_cov, clips)
    return len(km)


def test_reference_vector_k95_through_assemble_reads(rfx):
    """rfx_assemble_reads on the reads of chain_ds64_k95_P3_e8 gives the contig text and per-pass trace the reference's
    own classes made (`counter -kmer 95`, then `run -kmerc ... -kmer 95`)"""
    import reflexiv_amd
    z = np.load(T.VEC)
    name = "chain_ds64_k95_P3_e8"
    k, P, min_cov, mec, max_iter, min_iter, min_contig = [int(x) for x in z[name + "/meta"]]
    reads = bytes(z[name + "/reads"]).decode().split("\n")[:-1]
    bases, off = reads_of(reads)
    prm = reflexiv_amd.default_params(k=k, min_cov=min_cov, min_error_cov=mec, partitions=P, max_iter=max_iter,
                                      min_iter=min_iter, min_contig=min_contig)
    text, nc, trace, kept = rfx.assemble_reads(bases, off, prm)
    assert kept == len(z[name + "/asm_counts"])
    assert list(trace) == [int(x) for x in z[name + "/trace"]]
    assert text == bytes(z[name + "/contigs"]).decode()


@pytest.mark.parametrize("k", [65, 67, 81, 95, 97, 100, 127])
@pytest.mark.parametrize("clips", [(0, 0), (3, 5)])
def test_ragged_counts_match_the_oracle(rfx, torch_mod, k, clips):
    bases, off = ragged_reads_w(2000 + k, k)
    assert check_ragged(rfx, torch_mod, bases, off, k, clips=clips) > 0
    if clips == (0, 0):
        check_ragged(rfx, torch_mod, bases, off, k, min_covs=(1,), max_cov=4)


def test_edge_lengths_follow_the_counter64_skip_rule(rfx):
    for k in (65, 95, 97, 127):
        assert [rfx.kmers_per_read_w(n, k) for n in (k - 1, k, k + 1, k + 2)] == [0, 1, 2, 3]


def test_uniform_count_runs_the_leaf_kernels(rfx, torch_mod):
    """count_reads_w_dev at k = 95 goes through the bucketed count (its timing shows the leaves), not the sort path"""
    torch = torch_mod
    G, n, L, k = 50_000, 20_000, 150, 95
    og = O.synth_genome(17, G)
    bases, off = O.synth_reads(17, og, G, 0, n, L)
    dw, dl, nn, wpr, maxlen = upload(rfx, torch, np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(off, np.int64))
    cap = rfx.kmers_per_read_w(L, k) * n
    dk = torch.empty(cap * 3, dtype=torch.int64, device="cuda"); dc = torch.empty(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m, nd, inst = rfx.count_reads_w_dev(dw.data_ptr(), n, wpr, L, k, dk.data_ptr(), dc.data_ptr(), cap, 2)
    t = rfx.count_timing()
    assert t.get("leaf", (0, 0))[1] > 0 and "count_w" not in t and "extract_w" not in t, t
    wk, wc, wd = O.count_filter_w(O.extract_canon_w(bases, off, k), k, 2)
    assert (m, nd, inst) == (len(wk), wd, cap)
    assert np.array_equal(dk[:3 * m].cpu().numpy().view(np.uint64).reshape(m, 3), wk)
    assert np.array_equal(dc[:m].cpu().numpy(), wc)


def t_and_a_run_reads(k, uniform_len=None):
    """1200 reads of runs of 30..79 T's and A's, short mixed runs and random stretches, on both strands; k..219 bases each, or
    uniform_len"""
    rng = np.random.default_rng(k)
    reads = []
    for i in range(1200):
        parts = []
        while sum(map(len, parts)) < 200:
            c = rng.integers(0, 4)
            if c == 0:
                parts.append("T" * int(rng.integers(30, 80)))
            elif c == 1:
                parts.append("A" * int(rng.integers(30, 80)))
            elif c == 2:
                parts.append("".join(rng.choice(list("AT"), size=int(rng.integers(1, 6)))))
            else:
                parts.append("".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 20)))))
        s = "".join(parts)[:uniform_len or int(rng.integers(k, 220))]
        reads.append(s if rng.random() < 0.5 else "".join(COMP[c] for c in reversed(s)))
    return reads_of(reads)


@pytest.mark.parametrize("k", [67, 95, 100, 127])
def test_all_ones_and_all_zeros_middle_words(rfx, torch_mod, k):
    """runs of >= 32 T's and A's (and mixed runs) on both strands, so that word 1 (and word 2 at W = 4) -- and, from k = 64
    on, word 0 -- is all ones or all zeros: such keys must never share a table slot (the leaves claim slots by the last
    word, which is never all ones)"""
    bases, off = t_and_a_run_reads(k)
    km = O.extract_canon_w(bases, off, k)
    W = k // 32 + 1
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    for w in range(W - 1):
        assert (km[:, w] == ones).any() and (km[:, w] == 0).any(), w
    check_ragged(rfx, torch_mod, bases, off, k)
    # the same k-mers as host arrays (rfx_count_filter_w: the count straight from AoS elements)
    keys, counts, nd = rfx.groupBy_count_filter_w(km, k, 1)
    wk, wc, wd = O.count_filter_w(km, k, 1)
    assert np.array_equal(np.asarray(keys).reshape(-1, W), wk) and np.array_equal(np.asarray(counts), wc) and nd == wd


@pytest.mark.parametrize("env", [{"RFX_LEVEL_BITS": "4,3,3"},
                                 {"RFX_LEAF_TARGET": "200000", "RFX_WIDE_PRESPLIT": "64"},
                                 {"RFX_LEAF_TARGET": "200000", "RFX_WIDE_PRESPLIT": "100000000"}])
def test_leaf_tables_under_forced_plans(rfx, torch_mod, env, monkeypatch):
    """a distinct-heavy set (2 % substitutions) under several levels, leaves far beyond one table started in parts, and the
    same leaves found too full one pass at a time: counts equal the oracle's, and the leaves did split"""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    k = 95
    bases, off = ragged_reads_w(55, k, n_reads=8000, genome_len=40_000, err=0.02)
    check_ragged(rfx, torch_mod, bases, off, k, min_covs=(1,), clips=(2, 1))
    t = rfx.count_timing()
    if "RFX_LEAF_TARGET" in env:
        assert t["stat_passes"][1] > t["stat_leaves"][1] and t["stat_overflows"][1] > 0, t
    else:
        assert t["stat_leaves"][1] == 1 << 10 and t["stat_passes"][1] >= t["stat_leaves"][1], t


def test_junk_past_each_reads_length_is_never_read(rfx, torch_mod):
    """random bits past every read's length give the same counts as the zeros rfx_dev_encode_reads writes there"""
    torch = torch_mod
    k = 95
    bases, off = ragged_reads_w(5, k, n_reads=4000, genome_len=30_000)
    dw, dl, n, wpr, maxlen = upload(rfx, torch, bases, off)
    km = O.extract_canon_w(bases, off, k)
    want = count_ragged(rfx, torch, dw, dl, n, wpr, maxlen, k, len(km), 1)
    words = dw.cpu().numpy().view(np.uint64).reshape(n, wpr).copy()
    lens = off[1:] - off[:-1]
    rng = np.random.default_rng(6)
    junk = rng.integers(0, 1 << 63, size=words.shape, dtype=np.int64).view(np.uint64) * np.uint64(2) + np.uint64(1)
    for r in range(n):
        full, rem = divmod(int(lens[r]), 32)
        if rem:
            keep = ~np.uint64(0) << np.uint64(2 * (32 - rem))
            words[r, full] = (words[r, full] & keep) | (junk[r, full] & ~keep)
            full += 1
        words[r, full:] = junk[r, full:]
    dj = torch.from_numpy(words.reshape(-1).view(np.int64).copy()).cuda()
    got = count_ragged(rfx, torch, dj, dl, n, wpr, maxlen, k, len(km), 1)
    assert got[:3] == want[:3] and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    wk, wc, wd = O.count_filter_w(km, k, 1)
    assert np.array_equal(got[3], wk) and np.array_equal(got[4], wc)


@pytest.mark.parametrize("k", [81, 97])
def test_uniform_reads_through_the_ragged_entry(rfx, torch_mod, k):
    torch = torch_mod
    G, n, L = 100_000, 30_000, 150
    W = k // 32 + 1
    wpr = (L + 31) // 32
    dg = torch.empty((G + 31) // 32, dtype=torch.int64, device="cuda")
    dw = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    dl = torch.full((n,), L, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rfx.synth_genome_dev(3, G, dg.data_ptr())
    rfx.synth_reads_dev(3, dg.data_ptr(), G, 0, n, L, wpr, dw.data_ptr())
    rfx.sync()
    cap = rfx.kmers_per_read_w(L, k) * n
    ak = torch.empty(cap * W, dtype=torch.int64, device="cuda"); ac = torch.empty(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m0, nd0, inst0 = rfx.count_reads_w_dev(dw.data_ptr(), n, wpr, L, k, ak.data_ptr(), ac.data_ptr(), cap, 2)
    m, nd, inst, keys, counts = count_ragged(rfx, torch, dw, dl, n, wpr, L, k, cap, 2)
    assert (m, nd, inst) == (m0, nd0, inst0) and m > 0
    assert np.array_equal(keys, ak[:W * m].cpu().numpy().view(np.uint64).reshape(m, W))
    assert np.array_equal(counts, ac[:m].cpu().numpy())


def two_step(bases, off, k, cover, P, min_contig=100):
    wk, wc, _ = O.count_filter_w(O.extract_canon_w(bases, off, k), k, cover)
    text, nc, trace, _ = O.assemble_from_counts(O.counter_to_asm_w(wk, k), wc.astype(np.int32),
                                                O.default_params(k=k, min_cov=cover, partitions=P, min_contig=min_contig))
    return text, nc, trace, len(wk)


@pytest.mark.parametrize("k", [65, 95, 97, 124, 125])
@pytest.mark.parametrize("P", [1, 4])
def test_assemble_reads_matches_the_two_step_route(rfx, k, P):
    """ragged reads, and reads of one length (synthesised), against the oracle's counter -> KmerBinarizer -> driver"""
    import reflexiv_amd
    prm = reflexiv_amd.default_params(k=k, min_cov=2, partitions=P, min_contig=100)
    bases, off = ragged_reads_w(40 + k, k, n_reads=3000, genome_len=12_000)
    text, nc, trace, kept = rfx.assemble_reads(bases, off, prm)
    assert (text, nc, trace, kept) == two_step(bases, off, k, 2, P) and nc > 0
    og = O.synth_genome(8 + k, 20_000)
    ub, uo = O.synth_reads(8 + k, og, 20_000, 0, 3000, 150)
    ub, uo = np.ascontiguousarray(ub, np.uint8), np.ascontiguousarray(uo, np.int64)
    text, nc, trace, kept = rfx.assemble_reads(ub, uo, prm)
    assert (text, nc, trace, kept) == two_step(ub, uo, k, 2, P) and nc > 0


@pytest.mark.parametrize("k", [65, 95, 125])
def test_assemble_reads_without_k_mers(rfx, k):
    import reflexiv_amd
    prm = reflexiv_amd.default_params(k=k, min_cov=1, partitions=2)
    text, nc, trace, kept = rfx.assemble_reads(np.zeros(0, np.uint8), np.zeros(1, np.int64), prm)
    assert (text, nc, kept) == ("", 0, 0)
    rng = np.random.default_rng(2)
    bases, off = reads_of(["".join(rng.choice(list("ACGT"), size=int(L))) for L in rng.integers(0, k, size=500)])
    text, nc, trace, kept = rfx.assemble_reads(bases, off, prm)
    assert (text, nc, kept) == ("", 0, 0)


@pytest.mark.parametrize("sharded", [False, True])
def test_cli_run_resident_k95_equals_counter_then_run_kmerc(tmp_path, sharded):
    host, k = host_bin(), 95
    bases, off = ragged_reads_w(21, k, n_reads=4000, genome_len=15_000)
    fq = str(tmp_path / "r.fq")
    write_fq(fq, bases, off)
    cnt, two, one = str(tmp_path / "cnt"), str(tmp_path / "two"), str(tmp_path / "one")
    common = ["-kmer", str(k), "-cover", "2", "-mincontig", "100", "--logical-partitions", "4"]
    subprocess.check_call([host, "counter", "-fastq", fq, "-outfile", cnt, "-kmer", str(k), "-cover", "2"], timeout=600)
    subprocess.check_call([host, "run", "-kmerc", os.path.join(cnt, f"Count_{k}"), "-outfile", two] + common, timeout=600)
    env = dict(os.environ)
    if sharded:
        env["RFX_HOST_FORCE_SHARDED"] = "1"
    subprocess.check_call([host, "run", "--resident", "-fastq", fq, "-outfile", one] + common, env=env, timeout=600)
    want = open(os.path.join(two, f"Assemble_{k}", "part-00000"), "rb").read()
    assert want.startswith(b">Contig-")
    assert open(os.path.join(one, f"Assemble_{k}", "part-00000"), "rb").read() == want


@pytest.mark.parametrize("k,uniform", [(81, False), (97, False), (95, True)])
def test_cli_counter_resident_equals_counter(tmp_path, k, uniform):
    host = host_bin()
    if uniform:
        og = O.synth_genome(12, 20_000)
        bases, off = O.synth_reads(12, og, 20_000, 0, 3000, 150)
        bases, off = np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(off, np.int64)
    else:
        bases, off = ragged_reads_w(23 + k, k, n_reads=4000, genome_len=15_000)
    fq = str(tmp_path / "r.fq")
    write_fq(fq, bases, off)
    plain, dev = str(tmp_path / "plain"), str(tmp_path / "dev")
    args = ["-fastq", fq, "-kmer", str(k), "-cover", "2"]
    subprocess.check_call([host, "counter", "-outfile", plain] + args, timeout=600)
    subprocess.check_call([host, "counter", "--resident", "-outfile", dev] + args, timeout=600)
    want = open(os.path.join(plain, f"Count_{k}", "part-00000.csv"), "rb").read()
    assert want.count(b"\n") > 100
    assert open(os.path.join(dev, f"Count_{k}", "part-00000.csv"), "rb").read() == want
