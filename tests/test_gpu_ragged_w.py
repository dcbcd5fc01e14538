"""Reads of different lengths at k = 33..63 on the device: rfx_dev_count_reads_ragged_w against the oracle's k > 31 counter
(P/ReflexivDataFrameCounter64.java: its skip rule len - k - endClip + 1 <= 0, so reads of k and k + 1 bases emit one and two
k-mers), rfx_assemble_reads at k > 31 against the two-step route of the reference (`counter -kmer K`, then
`run -kmerc ... -kmer K`), and that route's CLI twin `run --resident -kmer 63`.  Bit-exact (integer work)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu


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


def ragged_reads(seed, k, n_reads=3000, genome_len=20_000, lower=True):
    """seeded reads of the edge lengths around k and 64 / 96, and random lengths up to 251, with N and lower case"""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), size=genome_len))
    edge = [0, 1, k - 2, k - 1, k, k + 1, k + 2, 64, 65, 96, 97, 150, 251]
    reads = []
    for i in range(n_reads):
        L = edge[i % len(edge)] if i < 4 * len(edge) else int(rng.integers(k - 3, 252))
        p = int(rng.integers(0, genome_len - L))
        s = list(genome[p:p + L])
        if L and rng.random() < 0.05:
            s[int(rng.integers(0, L))] = "N"
        if lower and L and rng.random() < 0.05:
            j = int(rng.integers(0, L))
            s[j] = s[j].lower()
        if rng.random() < 0.5:
            comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "n": "n", "a": "t", "c": "g", "g": "c", "t": "a"}
            s = [comp[c] for c in reversed(s)]
        reads.append("".join(s))
    bases = np.frombuffer("".join(reads).encode(), np.uint8).copy()
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.int64)
    return bases, off


def upload(rfx, torch, bases, off):
    """encode on the device -> (d_words, d_len, n, wpr, maxlen)"""
    n = len(off) - 1
    maxlen = int(max(1, (off[1:] - off[:-1]).max())) if n else 1
    wpr = (maxlen + 31) // 32
    db = torch.from_numpy(bases.copy() if len(bases) else np.zeros(1, np.uint8)).cuda()
    do = torch.from_numpy(off.copy()).cuda()
    dw = torch.empty(max(1, n * wpr), dtype=torch.int64, device="cuda")
    dl = torch.empty(max(1, n), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rfx.encode_reads_dev(db.data_ptr(), do.data_ptr(), n, wpr, dw.data_ptr(), dl.data_ptr())
    rfx.sync()
    return dw, dl, n, wpr, maxlen


def ragged_count(rfx, torch, dw, dl, n, wpr, maxlen, k, cap, min_cov=2, clips=(0, 0)):
    dk = torch.empty(max(1, cap) * 2, dtype=torch.int64, device="cuda")
    dc = torch.empty(max(1, cap), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m, nd, inst = rfx.count_reads_ragged_w_dev(dw.data_ptr(), dl.data_ptr(), n, wpr, maxlen, k, dk.data_ptr(), dc.data_ptr(),
                                               max(1, cap), min_cov, front_clip=clips[0], end_clip=clips[1])
    return m, nd, inst, dk[:2 * m].cpu().numpy().view(np.uint64).reshape(m, 2), dc[:m].cpu().numpy()


def test_edge_lengths_follow_the_counter64_skip_rule(rfx):
    """a read of k (k + 1) bases emits 1 (2) k-mers at k > 31 and none at k <= 31 (host arithmetic of both rules)"""
    for k in (33, 47, 62, 63):
        assert [rfx.kmers_per_read_w(n, k) for n in (k - 1, k, k + 1, k + 2)] == [0, 1, 2, 3]
    assert [rfx.kmers_per_read(n, 31) for n in (31, 32, 33)] == [0, 0, 3]


@pytest.mark.parametrize("k", [33, 47, 62, 63])
@pytest.mark.parametrize("clips", [(0, 0), (3, 5)])
def test_ragged_counts_match_the_oracle(rfx, torch_mod, k, clips):
    torch = torch_mod
    bases, off = ragged_reads(1000 + k, k)
    dw, dl, n, wpr, maxlen = upload(rfx, torch, bases, off)
    km = O.extract_canon_w(bases, off, k, *clips)
    for min_cov in (1, 2):
        m, nd, inst, keys, counts = ragged_count(rfx, torch, dw, dl, n, wpr, maxlen, k, len(km), min_cov, clips)
        wk, wc, wd = O.count_filter_w(km, k, min_cov)
        assert (inst, nd, m) == (len(km), wd, len(wk))
        assert np.array_equal(keys, wk) and np.array_equal(counts, wc)


def test_reads_of_exactly_k_and_k_plus_one(rfx, torch_mod):
    """the k > 31 rule pinned on reads that emit one and two k-mers (none of them would at k <= 31)"""
    torch = torch_mod
    k = 63
    rng = np.random.default_rng(9)
    reads = ["".join(rng.choice(list("ACGT"), size=L)) for L in (k, k + 1, k - 1, k, k + 1)]
    bases = np.frombuffer("".join(reads).encode(), np.uint8).copy()
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.int64)
    dw, dl, n, wpr, maxlen = upload(rfx, torch, bases, off)
    m, nd, inst, keys, counts = ragged_count(rfx, torch, dw, dl, n, wpr, maxlen, k, 16, 1)
    assert inst == 1 + 2 + 0 + 1 + 2
    wk, wc, wd = O.count_filter_w(O.extract_canon_w(bases, off, k), k, 1)
    assert np.array_equal(keys, wk) and np.array_equal(counts, wc) and nd == wd


@pytest.mark.parametrize("env", [{"RFX_LEVEL_BITS": "9,3"}, {"RFX_LEVEL_BITS": "9,2", "RFX_SK_ONESWEEP": "2"},
                                 {"RFX_WIDE_RECORDS": "0"}])
def test_ragged_counts_under_forced_plans(rfx, torch_mod, env, monkeypatch):
    """several record levels, level 1 in one sweep (its sampled histogram on ragged reads), and RFX_WIDE_RECORDS=0 -- which
    ragged reads do not follow: they always take the record path (the element path reads every read as the longest)"""
    torch = torch_mod
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    k = 63
    bases, off = ragged_reads(77, k, n_reads=12_000, genome_len=60_000)
    dw, dl, n, wpr, maxlen = upload(rfx, torch, bases, off)
    km = O.extract_canon_w(bases, off, k, 2, 1)
    m, nd, inst, keys, counts = ragged_count(rfx, torch, dw, dl, n, wpr, maxlen, k, len(km), 2, (2, 1))
    wk, wc, wd = O.count_filter_w(km, k, 2)
    assert (inst, nd, m) == (len(km), wd, len(wk))
    assert np.array_equal(keys, wk) and np.array_equal(counts, wc)


@pytest.mark.parametrize("k", [33, 63])
def test_uniform_reads_through_the_ragged_entry(rfx, torch_mod, k):
    """reads of one length through rfx_dev_count_reads_ragged_w give exactly rfx_dev_count_reads_w's output"""
    torch = torch_mod
    G, n, L = 100_000, 40_000, 150
    wpr = (L + 31) // 32
    dg = torch.empty((G + 31) // 32, dtype=torch.int64, device="cuda")
    dw = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    dl = torch.full((n,), L, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rfx.synth_genome_dev(3, G, dg.data_ptr())
    rfx.synth_reads_dev(3, dg.data_ptr(), G, 0, n, L, wpr, dw.data_ptr())
    rfx.sync()
    cap = rfx.kmers_per_read_w(L, k) * n
    ak = torch.empty(cap * 2, dtype=torch.int64, device="cuda"); ac = torch.empty(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m0, nd0, inst0 = rfx.count_reads_w_dev(dw.data_ptr(), n, wpr, L, k, ak.data_ptr(), ac.data_ptr(), cap, 2)
    m, nd, inst, keys, counts = ragged_count(rfx, torch, dw, dl, n, wpr, L, k, cap, 2)
    assert (m, nd, inst) == (m0, nd0, inst0) and m > 0
    assert np.array_equal(keys, ak[:2 * m].cpu().numpy().view(np.uint64).reshape(m, 2))
    assert np.array_equal(counts, ac[:m].cpu().numpy())


def test_junk_past_each_reads_length_is_never_read(rfx, torch_mod):
    """the contract of the header: random bits in every word (and every base slot of the last word) past a read's length
    give the same counts as the zeros rfx_dev_encode_reads writes there"""
    torch = torch_mod
    k = 63
    bases, off = ragged_reads(5, k, n_reads=6000, genome_len=40_000)
    dw, dl, n, wpr, maxlen = upload(rfx, torch, bases, off)
    km = O.extract_canon_w(bases, off, k)
    want = ragged_count(rfx, torch, dw, dl, n, wpr, maxlen, k, len(km), 1)
    words = dw.cpu().numpy().view(np.uint64).reshape(n, wpr).copy()
    lens = off[1:] - off[:-1]
    rng = np.random.default_rng(6)
    junk = rng.integers(0, 1 << 63, size=words.shape, dtype=np.int64).view(np.uint64) * np.uint64(2) + np.uint64(1)
    for r in range(n):
        full, rem = divmod(int(lens[r]), 32)
        if rem:
            keep = ~np.uint64(0) << np.uint64(2 * (32 - rem))                 # base i of a word in bits 63-2i, 62-2i
            words[r, full] = (words[r, full] & keep) | (junk[r, full] & ~keep)
            full += 1
        words[r, full:] = junk[r, full:]
    assert not np.array_equal(words, dw.cpu().numpy().view(np.uint64).reshape(n, wpr))
    dj = torch.from_numpy(words.reshape(-1).view(np.int64).copy()).cuda()
    got = ragged_count(rfx, torch, dj, dl, n, wpr, maxlen, k, len(km), 1)
    assert got[:3] == want[:3] and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    wk, wc, wd = O.count_filter_w(km, k, 1)
    assert np.array_equal(got[3], wk) and np.array_equal(got[4], wc)


def two_step(bases, off, k, cover, P, min_contig=100):
    """the reference's route at k > 31: counter (count + filter), KmerBinarizer + filter, assemblyFromKmer"""
    wk, wc, _ = O.count_filter_w(O.extract_canon_w(bases, off, k), k, cover)
    text, nc, trace, _ = O.assemble_from_counts(O.counter_to_asm_w(wk, k), wc.astype(np.int32),
                                                O.default_params(k=k, min_cov=cover, partitions=P, min_contig=min_contig))
    return text, nc, trace, len(wk)


@pytest.mark.parametrize("k", [33, 63])
@pytest.mark.parametrize("P", [1, 4])
def test_assemble_reads_ragged_matches_the_two_step_route(rfx, k, P):
    import reflexiv_amd
    bases, off = ragged_reads(40 + k, k, n_reads=4000, genome_len=15_000)
    text, nc, trace, kept = rfx.assemble_reads(bases, off, reflexiv_amd.default_params(k=k, min_cov=2, partitions=P, min_contig=100))
    otext, onc, otrace, okept = two_step(bases, off, k, 2, P)
    assert kept == okept and trace == otrace and nc == onc and text == otext
    assert nc > 0


@pytest.mark.parametrize("k", [33, 63])
def test_assemble_reads_uniform_matches_the_composed_device_path(rfx, torch_mod, k):
    """reads of one length: count_reads_w_dev -> counter_to_asm_dev -> assemble_w_dev, and the oracle"""
    import reflexiv_amd
    torch = torch_mod
    G, n, L, cover, P = 30_000, 6000, 150, 3, 4
    og = O.synth_genome(8, G)
    bases, off = O.synth_reads(8, og, G, 0, n, L)
    prm = reflexiv_amd.default_params(k=k, min_cov=cover, partitions=P, min_contig=100)
    text, nc, trace, kept = rfx.assemble_reads(bases, off, prm)
    dw, dl, nn, wpr, maxlen = upload(rfx, torch, np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(off, np.int64))
    cap = rfx.kmers_per_read_w(L, k) * n
    dk = torch.empty(cap * 2, dtype=torch.int64, device="cuda"); dc = torch.empty(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m, _, _ = rfx.count_reads_w_dev(dw.data_ptr(), n, wpr, L, k, dk.data_ptr(), dc.data_ptr(), cap, cover)
    ak = torch.empty(max(1, m) * O.asm_words(k), dtype=torch.int64, device="cuda"); ac = torch.empty(max(1, m), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m2 = rfx.counter_to_asm_dev(dk.data_ptr(), dc.data_ptr(), m, k, ak.data_ptr(), ac.data_ptr(), cover)
    wtext, wnc, wtrace = rfx.assemble_w_dev(ak.data_ptr(), ac.data_ptr(), m2, prm)
    assert (text, nc, trace, kept) == (wtext, wnc, wtrace, m2)
    otext, onc, otrace, okept = two_step(bases, off, k, cover, P)
    assert (text, nc, trace, kept) == (otext, onc, otrace, okept) and nc > 0


@pytest.mark.parametrize("k", [33, 63])
def test_assemble_reads_without_k_mers(rfx, k):
    """no reads, and reads that are all shorter than k: no contigs and no error"""
    import reflexiv_amd
    prm = reflexiv_amd.default_params(k=k, min_cov=1, partitions=2)
    text, nc, trace, kept = rfx.assemble_reads(np.zeros(0, np.uint8), np.zeros(1, np.int64), prm)
    assert (text, nc, kept) == ("", 0, 0)
    rng = np.random.default_rng(2)
    reads = ["".join(rng.choice(list("ACGT"), size=int(L))) for L in rng.integers(0, k, size=500)]
    bases = np.frombuffer("".join(reads).encode(), np.uint8).copy()
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.int64)
    text, nc, trace, kept = rfx.assemble_reads(bases, off, prm)
    assert (text, nc, kept) == ("", 0, 0)


def host_bin():
    import reflexiv_amd._lib as L
    return os.path.join(os.path.dirname(L.LIB_PATH), "reflexiv_host")


def write_fq(path, bases, off):
    with open(path, "w") as f:
        for i in range(len(off) - 1):
            s = bytes(bases[off[i]:off[i + 1]]).decode()
            f.write(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n")


@pytest.mark.parametrize("sharded", [False, True])
def test_cli_run_resident_k63_equals_counter_then_run_kmerc(tmp_path, sharded):
    host, k = host_bin(), 63
    bases, off = ragged_reads(21, k, n_reads=4000, genome_len=15_000)
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


def test_cli_run_k63_without_resident_still_needs_kmerc(tmp_path):
    bases, off = ragged_reads(22, 63, n_reads=50)
    fq = str(tmp_path / "r.fq")
    write_fq(fq, bases, off)
    r = subprocess.run([host_bin(), "run", "-fastq", fq, "-outfile", str(tmp_path / "o"), "-kmer", "63"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "-kmerc" in r.stderr


@pytest.mark.parametrize("k,uniform", [(63, False), (33, False), (63, True)])
def test_cli_counter_resident_equals_counter(tmp_path, k, uniform):
    """`counter --resident -kmer K` counts the packed reads on the device (rfx_dev_count_reads_ragged_w, or
    rfx_dev_count_reads_w when every read has one length) and writes Count_<k>/part-00000.csv byte for byte as `counter`"""
    host = host_bin()
    if uniform:
        og = O.synth_genome(12, 20_000)
        bases, off = O.synth_reads(12, og, 20_000, 0, 3000, 150)
        bases, off = np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(off, np.int64)
    else:
        bases, off = ragged_reads(23 + k, k, n_reads=4000, genome_len=15_000)
    fq = str(tmp_path / "r.fq")
    write_fq(fq, bases, off)
    plain, dev = str(tmp_path / "plain"), str(tmp_path / "dev")
    args = ["-fastq", fq, "-kmer", str(k), "-cover", "2"]
    subprocess.check_call([host, "counter", "-outfile", plain] + args, timeout=600)
    subprocess.check_call([host, "counter", "--resident", "-outfile", dev] + args, timeout=600)
    want = open(os.path.join(plain, f"Count_{k}", "part-00000.csv"), "rb").read()
    assert want.count(b"\n") > 100
    assert open(os.path.join(dev, f"Count_{k}", "part-00000.csv"), "rb").read() == want
