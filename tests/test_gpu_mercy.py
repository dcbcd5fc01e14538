"""The mercy k-mer stage (rfx_dev_mercy_kmers, rfx_dev_mercy_to_text, rfx_mercy_text) on the device: every case
of the rows the reference's own classes made (tests/golden/mercy_vectors.npz) and the string model (tests/mercy_model.py, which
test_mercy_model.py holds to the same vectors) key for key and byte for byte through all three entry points; window counts and gaps
around a ballot round of 64; read lengths on the word edge; junk behind every read; read counts around a workgroup; solid sets on both
sides of every directory size, the keys 0 and 4^k - 1, one long bucket; the chains from the project's own counter and into the k-mer
sorting stage; the argument, capacity and text-buffer contracts; and all of it again with every allocation poisoned."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ksort_model as K
from tests import mercy_model as M
from tests.test_gpu_dynamic_packed import FILL, OK, E_ARG, E_CAP
from tests.test_gpu_ksort import upload, text_of
from tests.test_gpu_map import dev_reads
from tests.test_mercy_model import GOLDEN, case_names, load_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


@pytest.fixture(scope="module")
def vectors():
    return np.load(GOLDEN)


def rand_seq(rng, n):
    return "".join("ACGT"[b] for b in rng.integers(0, 4, n))


def dev_keys(solid):
    """a set of k-mer strings -> (the sorted keys as a torch int64 tensor in HBM, their number)"""
    import torch
    keys = np.array(sorted(M.key_of(s) for s in solid), np.uint64)
    d = torch.from_numpy(np.concatenate([keys, np.zeros(1, np.uint64)]).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return d, len(keys)


def check(rfx, solid, reads, k, fc=0, ec=0, tag="", wpr=None, junk=None, rows=None, at_least=0, want_text=None):
    """the three entry points on one input against the string model -> the model's mercy k-mers"""
    want = M.mercy_kmers(reads, k, fc, ec, solid)
    assert len(want) >= at_least, (tag, len(want))
    text = "".join(f"{s},1\n" for s in want)
    assert want_text is None or text == want_text, (tag, "model against the vectors")
    dk, ns = dev_keys(solid)
    dw, dn, wpr = dev_reads(reads, wpr, junk)
    got = rfx.mercy_kmers(dk, ns, dw, dn, len(reads), wpr, k, fc, ec)
    assert rfx.last_call_ms > 0
    assert got.n == len(want), (tag, got.n, len(want))
    assert got.host().tolist() == [M.key_of(s) for s in want], (tag, "keys")
    t, ln, off = rfx.mercy_to_text(got.keys, got.n, k)
    assert bytes(t[:ln].cpu().numpy()).decode() == text, (tag, "text")
    assert off.cpu().tolist() == [i * (k + 3) for i in range(len(want) + 1)], (tag, "row offsets")
    rows = rows if rows is not None else [f"{s},2" for s in sorted(solid)][::-1]       # (a text file promises no order)
    host = rfx.mercy_text("".join(r + "\n" for r in rows).encode(), [r.encode() for r in reads], k, fc, ec)
    assert host.decode() == text, (tag, "host form")
    return want


def planted(rng, k, hit_sets, n):
    """reads of n bases each with the windows of one of hit_sets made solid -> (solid, reads)"""
    reads = [rand_seq(rng, n if isinstance(n, int) else n[i]) for i in range(len(hit_sets))]
    solid = {M.canon(r[p:p + k]) for r, hs in zip(reads, hit_sets) for p in hs}
    return solid, reads


# ---- 1. the reference's rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_every_case_of_the_reference(rfx, vectors, name):
    c = load_case(vectors, name)
    check(rfx, M.solid_set(c["rows"], c["k"]), c["reads"], c["k"], c["fc"], c["ec"], name, rows=c["rows"], want_text=c["text"])


# ---- 2. shapes around a ballot round ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 21, 31])
def test_window_counts_around_a_round_of_64(rfx, k):
    """window counts len - k + 1 of 1, 2, 3, 63, 64, 65, 127..129: the first and the last window solid (and one in the middle for the
    long ones), so the gap between them runs over the whole read"""
    rng = np.random.default_rng(k)
    counts = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129)
    hit_sets = [[0, w - 1] for w in counts] + [[0, w // 2, w - 1] for w in counts if w > 4]
    lens = [k + w - 1 for w in counts] + [k + w - 1 for w in counts if w > 4]
    solid, reads = planted(rng, k, hit_sets, lens)
    check(rfx, solid, reads, k, tag=("window counts", k), at_least=300)


@pytest.mark.parametrize("k", [15, 31])
def test_gaps_and_hits_that_straddle_windows_63_and_64(rfx, k):
    """a kept gap, a skipped gap (g = k) and a hit, each across the edge of a ballot round; gaps that end on 63 and start on 64; a gap
    that spans a whole round and two; both clips"""
    rng = np.random.default_rng(100 + k)
    hit_sets = [[60, 67], [60, 60 + k + 1], [63, 64], [62, 63, 64, 65], [50, 63], [64, 80], [63, 70], [57, 64], [63, 63 + k + 1], [64 - k - 1, 64],
                [10, 150], [10, 280], [63, 128], [0, 63, 64, 127, 128, 191, 192], [1, 64 + k, 130 + 2 * k]]
    solid, reads = planted(rng, k, hit_sets, 330)
    want = check(rfx, solid, reads, k, tag=("straddle", k), at_least=800)
    assert len(want) > 0
    check(rfx, solid, reads, k, 5, 7, tag=("straddle, clipped", k))
    check(rfx, solid, reads, k, 61, 40, tag=("straddle, clipped into the second round", k))


def test_read_lengths_on_the_word_edge_and_junk_behind_every_read(rfx):
    """reads of 32 words_per_read bases and one less; every bit behind a read's last base random, in its last word and in rows wider
    than any read"""
    rng = np.random.default_rng(7)
    for k in (16, 31):
        lens = [96, 95, 64, 63, 33, 32, 31, 70]
        hit_sets = [[0, 5, n - k] for n in lens]
        solid, reads = planted(rng, k, hit_sets, lens)
        check(rfx, solid, reads, k, tag=("word edge", k), wpr=3, junk=np.random.default_rng(8), at_least=100)
        check(rfx, solid, reads, k, tag=("wider rows", k), wpr=7, junk=np.random.default_rng(9))
        check(rfx, solid, reads, k, 0, 1, tag=("word edge, end clip 1", k), wpr=3, junk=np.random.default_rng(10))


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 513])
def test_read_counts_around_a_workgroup(rfx, n):
    rng = np.random.default_rng(n)
    k = 21
    hit_sets = [[2, int(rng.integers(4, 40)), 75] if i % 3 else [5] for i in range(n)]
    solid, reads = planted(rng, k, hit_sets, 100)
    check(rfx, solid or {"A" * k}, reads, k, tag=("reads", n), at_least=n if n >= 2 else 0)


def test_solid_sets_on_both_sides_of_every_directory_size(rfx):
    """n_solid of 0, 1, 2 and 2^j - 1, 2^j, 2^j + 1 up to 4,096; the keys 0 and 4^k - 1 among them"""
    rng = np.random.default_rng(5)
    k = 15
    base, reads = planted(rng, k, [[1, 9, 40], [0, 30, 80], [3, 4, 50]], 100)
    reads += ["C" + "A" * 20 + rand_seq(rng, 30) + "T" * 20 + "G", "G" + "T" * 16 + rand_seq(rng, 20) + "A" * 15 + "C"]      # windows of key 0
    pool = sorted({M.canon(rand_seq(rng, k)) for _ in range(4300)} - base)
    sizes = [0, 1, 2] + [n for j in range(2, 13) for n in (2 ** j - 1, 2 ** j, 2 ** j + 1)]
    for n in sizes:
        solid = set(sorted(base)[:n]) if n <= len(base) else base | set(pool[:n - len(base)])
        assert len(solid) == n
        check(rfx, solid, reads, k, tag=("n_solid", n), at_least=1 if n >= len(base) else 0)
    solid = base | {"A" * k, "T" * k} | set(pool[:100])          # the keys 0 and 4^k - 1 (a T run is never canonical: it matches nothing)
    want = check(rfx, solid, reads, k, tag="keys 0 and 4^k - 1", at_least=10)
    assert "A" * k not in want


def test_one_long_bucket(rfx):
    """300 solid keys that share their top 20 bits: the directory's one long bucket is searched by halves"""
    rng = np.random.default_rng(6)
    k = 31
    kmers = sorted({"A" * 10 + rand_seq(rng, 21) for _ in range(300)})
    assert len(kmers) == 300 and all(M.canon(s) == s for s in kmers) and len({M.key_of(s) >> 42 for s in kmers}) == 1
    reads = []
    for i in range(0, 300, 2):
        a, b = kmers[i], kmers[i + 1]
        reads.append("C" + a + rand_seq(rng, int(rng.integers(1, 50))) + (b if i % 4 else M.rc(b)) + "G")
    check(rfx, set(kmers), reads, k, tag="long bucket", at_least=2000)


def test_random_reads_against_random_solid_keys(rfx):
    """2,000 random reads against 5,000 random solid keys"""
    rng = np.random.default_rng(11)
    k = 21
    g = rand_seq(rng, 8000)
    all_k = sorted({M.canon(g[p:p + k]) for p in range(len(g) - k + 1)})
    solid = {all_k[i] for i in rng.permutation(len(all_k))[:5000]}
    reads = []
    for _ in range(2000):
        n = int(rng.integers(k - 2, 152))
        p = int(rng.integers(0, len(g) - n))
        r = g[p:p + n]
        reads.append(M.rc(r) if rng.integers(0, 2) else r)
    check(rfx, solid, reads, k, tag="random", at_least=10000)
    check(rfx, solid, reads, k, 3, 4, tag="random, clipped", at_least=10000)


# ---- 3. chains -------------------------------------------------------------------------------------------------------------------------
def count_on_device(rfx, reads, k, min_cov=2):
    """the project's own counter on the reads -> (dk, dc, survivors, the read store)"""
    import torch
    dw, dn, wpr = dev_reads(reads)
    cap = sum(max(0, len(r) - k + 1) for r in reads) + 1
    dk = torch.empty(cap, dtype=torch.int64, device="cuda")
    dc = torch.empty(cap, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m, _, _ = rfx.count_reads_ragged_dev(dw.data_ptr(), dn.data_ptr(), len(reads), wpr, max(len(r) for r in reads), k, dk.data_ptr(), dc.data_ptr(), cap, min_cov)
    return dk, dc, m, (dw, dn, wpr)


def kmer_of(key, k):
    return "".join("ACGT"[(int(key) >> (2 * (k - 1 - j))) & 3] for j in range(k))


def test_the_counter_into_the_mercy_stage_gives_the_genomes_stretches(rfx, vectors):
    """count_reads_ragged (min_cov 2) on the planted genome's reads -> mercy_kmers -> mercy_to_text: exactly the k-mers of the GENOME
    windows that touch a stretch of single coverage; and the host form and the vectors say the same"""
    c = load_case(vectors, "planted_k31")
    k = c["k"]
    genome = bytes(vectors["planted_k31/genome"]).decode()
    dk, dc, m, (dw, dn, wpr) = count_on_device(rfx, c["reads"], k)
    got = rfx.mercy_kmers(dk, m, dw, dn, len(c["reads"]), wpr, k)
    t, ln, _ = rfx.mercy_to_text(got.keys, got.n, k)
    text = bytes(t[:ln].cpu().numpy()).decode()
    want = [M.canon(genome[p:p + k]) for lo, hi in vectors["planted_k31/stretches"].tolist() for p in range(len(genome) - k + 1) if p + k > lo and p < hi]
    assert sorted(text.split()) == sorted(f"{s},1" for s in want) and len(want) > 100
    assert text == c["text"]
    count_rows = [f"{kmer_of(key, k)},{n}" for key, n in zip(dk[:m].cpu().numpy().view(np.uint64), dc[:m].cpu().numpy())]
    assert rfx.mercy_text("".join(r + "\n" for r in count_rows).encode(), [r.encode() for r in c["reads"]], k).decode() == text


def test_counter_rows_and_mercy_rows_into_the_kmer_sorting_stage(rfx, vectors):
    """the counter's rows followed by the mercy rows (the order Spark lists Count_31/ and Count_31_mercy/) -> ksort_run, the mercy
    text and its offsets straight from the device: the result equals ksort_model on the same rows"""
    import torch
    c = load_case(vectors, "planted_k31")
    k = c["k"]
    dk, dc, m, (dw, dn, wpr) = count_on_device(rfx, c["reads"], k)
    got = rfx.mercy_kmers(dk, m, dw, dn, len(c["reads"]), wpr, k)
    t, ln, off = rfx.mercy_to_text(got.keys, got.n, k)
    count_rows = [f"{kmer_of(key, k)},{n}\n" for key, n in zip(dk[:m].cpu().numpy().view(np.uint64), dc[:m].cpu().numpy())]
    ct, co = upload(count_rows)
    d_text = torch.cat([ct, t[:ln]])
    d_off = torch.cat([co, off[1:] + int(ct.numel())])
    torch.cuda.synchronize()
    p = K.default_params(k)
    cp = rfx.ksort_params(k)
    out = rfx.ksort_run(d_text, d_off, cp)
    rows = count_rows + [r + "\n" for r in bytes(t[:ln].cpu().numpy()).decode().split()]
    assert len(rows) == m + got.n and got.n > 100
    assert text_of(rfx, out, k) == K.run_text(rows, p)


def test_the_mercy_sub_command_and_sort_on_both_directories(vectors, tmp_path):
    """`reflexiv_host mercy` writes O/Count_<k>_mercy/part-00000.csv with the rows of the device chain (the vectors' text, which the
    chain test above equals); `sort -kmerc Count_31,Count_31_mercy` reads the parts in that order -- the order Spark lists them, '/'
    before '_' -- and equals `sort` on the concatenated file and the string model; without arguments `mercy` says what it needs"""
    c = load_case(vectors, "planted_k31")
    k = c["k"]
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    out = tmp_path / "out"
    d = out / f"Count_{k}"
    d.mkdir(parents=True)
    (d / "part-00000.csv").write_text("".join(r + "\n" for r in c["rows"]))
    fq = tmp_path / "reads.fq"
    fq.write_text("".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(c["reads"])))
    r = subprocess.run([exe, "mercy", "-kmerc", str(d), "-fastq", str(fq), "-kmer", str(k), "-outfile", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    md = out / f"Count_{k}_mercy"
    assert (md / "part-00000.csv").read_text() == c["text"] and (md / "_SUCCESS").exists()
    r = subprocess.run([exe, "mercy"], capture_output=True, text=True)
    assert r.returncode != 0 and "-kmerc" in r.stderr and "-fastq" in r.stderr and "-kmer" in r.stderr
    r = subprocess.run([exe, "mercy", "-kmerc", str(d), "-fastq", str(fq), "-kmer", "33", "-outfile", str(out)], capture_output=True, text=True)
    assert r.returncode != 0 and "8..31" in r.stderr
    both = tmp_path / "both.csv"
    both.write_text((d / "part-00000.csv").read_text() + c["text"])
    texts = []
    for i, src in enumerate((f"{d},{md}", str(both), str(d))):
        o = tmp_path / f"sorted{i}"
        r = subprocess.run([exe, "sort", "-kmerc", src, "-kmer", str(k), "-outfile", str(o)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        texts.append((o / f"Count_{k}_sorted" / "part-00000.csv").read_text())
    assert texts[0] == texts[1] == K.run_text([r + "\n" for r in c["rows"]] + c["text"].splitlines(True), K.default_params(k))
    assert texts[2] == K.run_text([r + "\n" for r in c["rows"]], K.default_params(k)) and texts[2] != texts[0]


# ---- 4. contracts ----------------------------------------------------------------------------------------------------------------------
def small_input(rfx, k=21):
    rng = np.random.default_rng(3)
    solid, reads = planted(rng, k, [[1, 30], [0, 50, 60], [7]], 100)
    dk, ns = dev_keys(solid)
    dw, dn, wpr = dev_reads(reads)
    return solid, reads, dk, ns, dw, dn, wpr, len(M.mercy_kmers(reads, k, 0, 0, solid))


def filled(n, dtype):
    import torch
    t = torch.empty(max(1, n), dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    return t


def untouched(t):
    import torch
    return bool((t.view(torch.uint8) == FILL).all())


def raw_kmers(rfx, dk, ns, dw, dn, nr, wpr, k, fc, ec, out, cap, n):
    p = lambda t: t.data_ptr() if t is not None else None       # noqa: E731
    return rfx.L.rfx_dev_mercy_kmers(rfx.ctx, p(dk), ns, p(dw), p(dn), nr, wpr, k, fc, ec, p(out), cap, C.addressof(n) if n is not None else None)


def test_every_refused_argument_leaves_the_outputs_untouched(rfx):
    import torch
    k = 21
    solid, reads, dk, ns, dw, dn, wpr, need = small_input(rfx, k)
    out = filled(need + 8, torch.int64)
    n = C.c_int64(-77)
    ok = dict(dk=dk, ns=ns, dw=dw, dn=dn, nr=len(reads), wpr=wpr, k=k, fc=0, ec=0, out=out, cap=need + 8, n=n)
    bad = [dict(k=7), dict(k=32), dict(k=0), dict(fc=-1), dict(ec=-1), dict(wpr=0), dict(wpr=938), dict(dk=None), dict(dw=None), dict(dn=None),
           dict(out=None), dict(n=None), dict(ns=-1), dict(nr=-1), dict(cap=-1)]
    for b in bad:
        assert raw_kmers(rfx, **{**ok, **b}) == E_ARG, b
        assert untouched(out) and n.value == -77, b
    # solid keys that descend, repeat, or reach 4^k; a read length the words do not hold, and one of 30000
    keys = np.array(sorted(M.key_of(s) for s in solid), np.uint64)
    for name, ks in (("descending", keys[::-1]), ("duplicate", np.concatenate([keys[:2], keys[1:]])), ("not below 4^k", np.concatenate([keys, [np.uint64(1) << np.uint64(2 * k)]])),
                     ("descending at the end", np.concatenate([keys, keys[-1:] - np.uint64(1)]))):
        d = torch.from_numpy(ks.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        assert raw_kmers(rfx, **{**ok, "dk": d, "ns": len(ks)}) == E_ARG, name
        assert untouched(out) and n.value == -77, name
        assert b"ascending" in rfx.L.rfx_last_error(rfx.ctx)
    for name, lens in (("above 32 words_per_read", [100, 32 * wpr + 1, 100]), ("30000", [100, 100, 30000]), ("2^32 - 1", [2 ** 32 - 1, 100, 100])):
        d = torch.from_numpy(np.array(lens, np.uint32).view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        assert raw_kmers(rfx, **{**ok, "dn": d}) == E_ARG, name
        assert untouched(out) and n.value == -77, name
    # a read length of 30000 with words_per_read 938: refused on the argument alone (no array of that shape is looked at)
    assert raw_kmers(rfx, **{**ok, "wpr": 938}) == E_ARG and untouched(out) and n.value == -77
    # the text entry point
    ln = C.c_int64(-77)
    txt = filled(64, torch.uint8)
    off = filled(8, torch.int64)
    T = rfx.L.rfx_dev_mercy_to_text
    for args in ((None, 2, k, txt.data_ptr(), 64, C.addressof(ln), off.data_ptr()), (out.data_ptr(), -1, k, txt.data_ptr(), 64, C.addressof(ln), off.data_ptr()),
                 (out.data_ptr(), 2, 7, txt.data_ptr(), 64, C.addressof(ln), off.data_ptr()), (out.data_ptr(), 2, 32, txt.data_ptr(), 64, C.addressof(ln), off.data_ptr()),
                 (out.data_ptr(), 2, k, None, 64, C.addressof(ln), off.data_ptr()), (out.data_ptr(), 2, k, txt.data_ptr(), -1, C.addressof(ln), off.data_ptr()),
                 (out.data_ptr(), 2, k, txt.data_ptr(), 64, None, off.data_ptr())):
        assert T(rfx.ctx, *args) == E_ARG, args
        assert untouched(txt) and untouched(off) and ln.value == -77
    # the host form: a row without a comma, a count that is not digits, a read of 30000 bases, k out of range
    from reflexiv_amd import RfxError
    good = "".join(f"{s},2\n" for s in sorted(solid)).encode()
    for rows, rd, kk in ((good + b"ACGT\n", reads, k), (good + b"ACGTACGTACGTACGTACGTA,x\n", reads, k), (good + b"ACGTACGTACGTACGTACGTA,-3\n", reads, k),
                         (good, reads + ["A" * 15 + "C" * 29985], k), (good, reads, 7), (good, reads, 32)):
        with pytest.raises(RfxError) as ei:
            rfx.mercy_text(rows, [r.encode() for r in rd], kk)
        assert ei.value.status == E_ARG
    with pytest.raises(RfxError) as ei:
        rfx.mercy_text(good, [r.encode() for r in reads], k, front_clip=-1)
    assert ei.value.status == E_ARG
    assert rfx.mercy_text(good, [r.encode() for r in reads + ["C" * 29999]], k).count(b"\n") == need      # (the longest read the stage takes)


def test_empty_inputs_are_valid(rfx):
    k = 21
    solid, reads, dk, ns, dw, dn, wpr, need = small_input(rfx, k)
    assert rfx.mercy_kmers(dk, 0, dw, dn, len(reads), wpr, k).n == 0
    assert rfx.mercy_kmers(dk, ns, dw, dn, 0, wpr, k).n == 0
    assert rfx.mercy_kmers(dk, 0, dw, dn, 0, wpr, k).n == 0
    t, ln, off = rfx.mercy_to_text(dk, 0, k)
    assert ln == 0 and off.cpu().tolist() == [0]
    assert rfx.mercy_text(b"", [r.encode() for r in reads], k) == b""
    assert rfx.mercy_text("".join(f"{s},2\n" for s in solid).encode(), [], k) == b""
    assert rfx.mercy_text(b"", [], k) == b""
    n = C.c_int64(-1)
    assert raw_kmers(rfx, None, 0, None, None, 0, 1, k, 0, 0, None, 0, n) == OK and n.value == 0


def test_a_short_capacity_reports_the_need_and_writes_nothing(rfx):
    import torch
    from reflexiv_amd.api import MercyKmers
    k = 21
    solid, reads, dk, ns, dw, dn, wpr, need = small_input(rfx, k)
    assert need > 10
    for cap in (need - 1, 0):
        out = filled(need, torch.int64)
        n = C.c_int64(-77)
        assert raw_kmers(rfx, dk, ns, dw, dn, len(reads), wpr, k, 0, 0, out, cap, n) == E_CAP
        assert n.value == need and untouched(out)
    n = C.c_int64(-77)
    assert raw_kmers(rfx, dk, ns, dw, dn, len(reads), wpr, k, 0, 0, None, 0, n) == E_CAP and n.value == need
    out = filled(need + 3, torch.int64)
    assert raw_kmers(rfx, dk, ns, dw, dn, len(reads), wpr, k, 0, 0, out, need, n) == OK and n.value == need
    assert untouched(out[need:]) and not untouched(out[:need])
    # a wrapper output of capacity 1 is replaced by one of the need
    got = rfx.mercy_kmers(dk, ns, dw, dn, len(reads), wpr, k, out=MercyKmers(1))
    assert got.n == need and got.cap_n == need
    assert got.host().tolist() == [M.key_of(s) for s in M.mercy_kmers(reads, k, 0, 0, solid)]


def test_the_text_buffer_rule_at_every_cap_with_an_unaligned_buffer(rfx):
    """filled up to cap, nothing at or past it, RFX_E_CAP with *out_len = the need, at every cap from 0 to the need and every residue
    of the destination address mod 16"""
    import torch
    for k in (8, 15, 31):
        rng = np.random.default_rng(k)
        kmers = [rand_seq(rng, k) for _ in range(5)]
        text = "".join(f"{s},1\n" for s in kmers).encode()
        need = len(text)
        keys = torch.from_numpy(np.array([M.key_of(s) for s in kmers], np.uint64).view(np.int64).copy()).cuda()
        for skew in (0, 1, 7, 15):
            buf = filled(need + 64, torch.uint8)
            assert buf.data_ptr() % 16 == 0
            for cap in list(range(0, need + 1)) + [need + 5]:
                buf.fill_(FILL)
                torch.cuda.synchronize()
                ln = C.c_int64(-1)
                st = rfx.L.rfx_dev_mercy_to_text(rfx.ctx, keys.data_ptr(), 5, k, buf.data_ptr() + skew if cap else None, cap, C.addressof(ln), None)
                assert st == (E_CAP if cap < need else OK) and ln.value == need, (k, skew, cap)
                got = bytes(buf.cpu().numpy())
                lim = min(cap, need)
                assert got[skew:skew + lim] == text[:lim] and set(got[:skew]) <= {FILL} and set(got[skew + lim:]) == {FILL}, (k, skew, cap)


def test_everything_again_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it, so a kernel that
    relied on zeroed memory fails the checks above.  A child process: the mask is read once per process."""
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned and not sub_command"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
