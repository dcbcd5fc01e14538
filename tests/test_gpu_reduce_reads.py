"""Reduce from reads in one resident call (rfx_dev_reduce_reads).  The expected set is always built by a Python
helper that chains the entry points that existed before it, with text between them: count_reads_ragged[_w]_dev, the rows printed from
the downloaded keys, mercy_text when sensitive, ksort_text, reduce_text pair by pair, dyn_binarize_dev form 0 over the concatenated
Count_<k>_reduced texts -- and the E rule applied per k in Python.  Sets are compared array by array, whole words.

That expected set comes from the library itself, so this file holds the driver to its own stages and the contracts of the call
(capacities, refused arguments, the command against its older modes).  What holds the call to something independent -- the composed string
models from the reads to the rows, on reads where a later k's E reaches the output and where the counter's second count runs -- is
tests/test_gpu_reduce_reads_model.py."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from tests.test_gpu_dynamic_packed import poisoned, untouched, FILL, E_ARG, E_CAP
from tests.test_gpu_ksort import upload
from tests.test_gpu_ksort_counts import same_set, NUC
from tests.test_gpu_map import dev_reads

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIST = (23, 31, 41, 53, 67, 81, 95)          # (the default list cut at 95)


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


def rnd(rng, m):
    return "".join(NUC[b] for b in rng.integers(0, 4, m))


@pytest.fixture(scope="module")
def synthetic():
    """a 2,000-base random genome with one 60-base repeat and one copy of a stretch with a planted SNP; reads of 120..150 bases at
    depth about 12 with 1 % substitutions.  Behind them a planted fork with exact counts: 12 reads of a 150-base sequence and 7 of
    its copy with one SNP at base 100, so that at every k of the lists one sub-k-mer has extensions of count 12 and 7 -- an error
    for E = 8 (7 <= 8 and 12 >= 1.5 * 7), a variant for E = 6"""
    rng = np.random.default_rng(20240611)
    g = list(rnd(rng, 2000))
    g[1400:1460] = g[300:360]
    g[1700:1850] = g[700:850]
    g[1775] = NUC[(NUC.index(g[1775]) + 1) % 4]
    g = "".join(g)
    reads = []
    while sum(len(r) for r in reads) < 12 * len(g):
        n = int(rng.integers(120, 151))
        p = int(rng.integers(0, len(g) - n + 1))
        r = [NUC[(NUC.index(c) + 1 + int(rng.integers(0, 3))) % 4] if rng.random() < 0.01 else c for c in g[p:p + n]]
        reads.append("".join(r))
    s = rnd(rng, 150)
    v = s[:100] + NUC[(NUC.index(s[100]) + 2) % 4] + s[101:]
    return reads + [s] * 12 + [v] * 7


def kmer_strings(keys, k):
    """the counter's keys ([n, k // 32 + 1] uint64) as their letters, as DSBinaryKmerToString prints them"""
    W = k // 32 + 1
    keys = keys.reshape(-1, W)
    cols = []
    for j in range(W):
        m = min(32, k - 32 * j)
        shifts = (2 * (m - 1 - np.arange(m))).astype(np.uint64)
        cols.append((keys[:, j:j + 1] >> shifts) & np.uint64(3))
    letters = np.frombuffer(b"ACGT", np.uint8)[np.concatenate(cols, axis=1).astype(np.uint8)]
    return [bytes(r).decode() for r in letters]


def count_rows(rfx, store, n_reads, max_len, k, prm):
    import torch
    dw, dn, wpr = store
    W = k // 32 + 1
    cap = n_reads * max(max_len - k + 1, 0) + 1
    dk = torch.empty(cap * W, dtype=torch.int64, device="cuda")
    dc = torch.empty(cap, dtype=torch.int32 if k <= 31 else torch.int64, device="cuda")
    torch.cuda.synchronize()
    fn = rfx.count_reads_ragged_dev if k <= 31 else rfx.count_reads_ragged_w_dev
    m, _, _ = fn(dw.data_ptr(), dn.data_ptr(), n_reads, wpr, max_len, k, dk.data_ptr(), dc.data_ptr(), cap, min_cov=prm.min_cov,
                 max_cov=prm.max_cov, front_clip=prm.front_clip, end_clip=prm.end_clip)
    keys = dk[:m * W].cpu().numpy().view(np.uint64)
    return [f"{s},{int(c)}\n" for s, c in zip(kmer_strings(keys, k), dc[:m].cpu().numpy())]


def e_rule(klist, prm):
    """minErrorCoverage per k: sticky; the first k sets 3 min_cov iff (k >= 61 and the second k < 81) or k >= 81, a later k iff k >= 61"""
    out, E = [], prm.min_error_cov
    for i, k in enumerate(klist):
        if ((k >= 61 and klist[1] < 81) or k >= 81) if i == 0 else k >= 61:
            E = 3 * prm.min_cov
        out.append(E)
    return out


def chain(rfx, reads, klist, prm, fixed_E=None):
    """the same work through the entry points that exist without the driver -> (the set of the first-four passes, each k's rows, the
    mercy rows that reached the sorter, the text of every Count_<k>_reduced)"""
    n_reads, max_len = len(reads), max([len(r) for r in reads] + [0])
    store = dev_reads(reads) if reads else None
    Es = [fixed_E] * len(klist) if fixed_E is not None else e_rule(klist, prm)
    reduced, prev, mercy = [], b"", 0
    for i, k in enumerate(klist):
        rows = "".join(count_rows(rfx, store, n_reads, max_len, k, prm)).encode() if reads else b""
        if prm.sensitive and k <= 31 and reads:
            extra = rfx.mercy_text(rows, [r.encode() for r in reads], k, prm.front_clip, prm.end_clip)
            mercy += extra.count(b"\n")
            rows += extra
        cp = rfx.ksort_params(k, max_k=klist[-1], min_error_cov=Es[i], max_cov=prm.max_cov, bubble=prm.bubble, min_repeat_fold=prm.min_repeat_fold)
        cur = rfx.ksort_text(rows, cp)
        if i == 0:
            prev = cur
            continue
        short, prev = rfx.reduce_text(prev, cur, prm.P, rfx.reduce_params(klist[i - 1], k, max_k=klist[-1]))
        reduced.append(short)
    reduced.append(prev)
    text = b"".join(reduced)
    rows = [r + "\n" for r in text.decode().split("\n") if r]
    return rfx.dyn_binarize_dev(*upload(rows), 0), [t.count(b"\n") for t in reduced], mercy, reduced


def driver(rfx, reads, klist, prm):
    if not reads:
        return rfx.reduce_reads_dev(None, None, 0, 1, 0, klist, prm)
    dw, dn, wpr = dev_reads(reads)
    return rfx.reduce_reads_dev(dw, dn, len(reads), wpr, max(len(r) for r in reads), klist, prm)


def check(rfx, reads, klist, tag, **kw):
    prm = rfx.reduce_reads_params(**kw)
    want, want_n, mercy, texts = chain(rfx, reads, klist, prm)
    got, got_n = driver(rfx, reads, klist, prm)
    assert got_n == want_n, (tag, got_n, want_n)
    same_set(got, want, tag)
    assert rfx.reduce_reads_text([r.encode() for r in reads], klist, prm) == texts, (tag, "reduce_reads_text")   # (byte for byte)
    return got, got_n, mercy


def test_the_example_reads(rfx):
    lines = gzip.open(os.path.join(HERE, "golden", "paired_dat1.fq.gz"), "rt").read().split("\n")
    reads = [s for s in lines[1::4] if s]
    got, per_k, _ = check(rfx, reads, (23, 31, 41), "paired_dat1", P=8)
    assert len(reads) == 1150 and got.n == sum(per_k) and min(per_k) > 0


@pytest.mark.parametrize("P", [1, 8])
@pytest.mark.parametrize("klist", [(31, 33), (23, 67, 95), (65, 81), (81, 95), DEFAULT_LIST], ids=lambda l: "k" + "_".join(map(str, l)))
def test_synthetic_reads_through_every_branch_of_the_e_rule(rfx, synthetic, klist, P):
    """(31, 33): never set; (23, 67, 95): set by a later k; (65, 81): the first k is 61 or more but the second is not below 81 -- the
    first-k quirk, E stays 8 for k = 65 and becomes 6 at 81; (81, 95): set by the first k; the default list: set at 67"""
    prm = rfx.reduce_reads_params(P=P)
    assert e_rule(klist, prm) == {(31, 33): [8, 8], (23, 67, 95): [8, 6, 6], (65, 81): [8, 6], (81, 95): [6, 6],
                                  DEFAULT_LIST: [8, 8, 8, 8, 6, 6, 6]}[klist]
    got, per_k, _ = check(rfx, synthetic, klist, (klist, P), P=P)
    assert got.n == sum(per_k) and min(per_k) > 0


def test_the_e_rule_changes_the_result(rfx, synthetic):
    """the list (81, 95) lies past 61, E = 6 from its first k on: the helper's chain with E fixed at 8 must give a DIFFERENT set, or
    the input is too weak to show that the rule is applied.  (The string models say the same of these reads: the planted fork's two
    95-mers end `1|98|-1` / `1|-1|98` under E = 6 and `1|-1|-1` under E = 8.  Behind a shorter k the reduction forces those markers to
    -1 either way, because this fork is an error at the short k too (7 <= 8), so on THESE reads the lists that start below 61 do not
    show a later k's E.  The `forked` reads of tests/reduce_reads_model.py do: tests/test_reduce_reads_model.py asserts which list
    separates which wrong rule, and tests/test_gpu_reduce_reads_model.py holds the driver to the model's texts on those lists.)"""
    klist = (81, 95)
    prm = rfx.reduce_reads_params(P=8)
    ruled, n_ruled, _, _ = chain(rfx, synthetic, klist, prm)
    fixed, n_fixed, _, _ = chain(rfx, synthetic, klist, prm, fixed_E=8)
    same = ruled.n == fixed.n and all(np.array_equal(a, b) for a, b in zip(ruled.host(), fixed.host()))
    assert not same, "E = 8 throughout gives the same set: the reads do not exercise the rule"
    got, got_n = driver(rfx, synthetic, klist, prm)
    same_set(got, ruled, "ruled")
    assert got_n == n_ruled


def test_sensitive_mode_brings_the_mercy_kmers_to_the_sorter(rfx):
    """reads with planted holes (tests/golden/mercy_vectors.npz `planted_k31`, made as tests/mercy_model.py describes): stretches of
    single coverage between solid k-mers; at least one mercy k-mer must reach the sorter, and the result must differ from the
    plain mode's"""
    from tests.test_mercy_model import GOLDEN, load_case
    reads = load_case(np.load(GOLDEN), "planted_k31")["reads"]
    got, per_k, mercy = check(rfx, reads, (23, 31, 41), "sensitive", sensitive=1, P=8)
    assert mercy > 0
    plain, plain_n = driver(rfx, reads, (23, 31, 41), rfx.reduce_reads_params(P=8))
    assert plain_n != per_k or plain.n != got.n


def test_other_parameters_reach_their_stages(rfx, synthetic):
    for kw in (dict(min_cov=3), dict(max_cov=11), dict(bubble=0), dict(front_clip=3, end_clip=5), dict(min_error_cov=5, min_repeat_fold=2.0)):
        check(rfx, synthetic, (31, 41, 67), kw, P=3, **kw)


def test_no_reads_and_reads_shorter_than_the_last_k(rfx):
    got, per_k, _ = check(rfx, [], (23, 31, 41), "no reads")
    assert got.n == 0 and per_k == [0, 0, 0] and int(got.ext_off[0]) == 0
    rng = np.random.default_rng(4)
    g = rnd(rng, 300)
    reads = [g[p:p + 60] for p in rng.integers(0, 241, 120)]
    got, per_k, _ = check(rfx, reads, (23, 31, 67), "short reads", P=3)
    assert per_k[2] == 0 and per_k[0] > 0


def raw_call(rfx, store, n_reads, max_len, klist, prm, co, per_k=None, n_k=None):
    dw, dn, wpr = store
    ks = (C.c_int * max(len(klist), 1))(*klist)
    per_k = per_k if per_k is not None else (C.c_int64 * 16)()
    return rfx.L.rfx_dev_reduce_reads(rfx.ctx, dw.data_ptr(), dn.data_ptr(), n_reads, wpr, max_len, C.addressof(ks), len(klist) if n_k is None else n_k,
                                      C.byref(prm) if prm is not None else None, C.byref(co) if co is not None else None, C.addressof(per_k))


def test_a_short_output_reports_the_need_and_writes_nothing(rfx, synthetic):
    klist = (23, 31)
    store = dev_reads(synthetic)
    max_len = max(len(r) for r in synthetic)
    prm = rfx.reduce_reads_params(P=3)
    got, per_k = driver(rfx, synthetic, klist, prm)
    need = got.n
    for cap_n, cap_w in ((need - 1, need), (need, need - 1), (0, 0)):
        d = poisoned(cap_n, cap_w)
        co = d._c()
        co.n = co.need_words = -77
        assert raw_call(rfx, store, len(synthetic), max_len, klist, prm, co) == E_CAP
        assert (int(co.n), int(co.need_words)) == (need, need) and untouched(d)
    d = poisoned(need, need)
    co = d._c()
    assert raw_call(rfx, store, len(synthetic), max_len, klist, prm, co) == 0 and int(co.n) == need
    d._take(co)
    same_set(d, got, "exact capacity")


def test_refused_arguments_write_nothing(rfx, synthetic):
    reads = synthetic[:40]
    store = dev_reads(reads)
    max_len = max(len(r) for r in reads)
    good = rfx.reduce_reads_params()
    d = poisoned(1 << 14, 1 << 14)

    def refused(klist, prm=good, n_k=None, st=None, n_reads=len(reads), ml=max_len):
        co = d._c()
        co.n = co.need_words = -77
        code = raw_call(rfx, st or store, n_reads, ml, klist, prm, co, n_k=n_k)
        return code == E_ARG and untouched(d) and (int(co.n), int(co.need_words)) == (-77, -77)

    assert refused((31,)) and refused(tuple(range(20, 37)), n_k=17) and refused((23, 31), n_k=0) and refused((23, 31), n_k=-1)
    assert refused((31, 31)) and refused((41, 31)) and refused((23, 41, 31))
    for bad in (7, 125, 32, 63, 94, 64, 96):
        assert refused((bad, 124) if bad < 124 else (23, bad)), bad
    for P in (0, 64, -1):
        assert refused((23, 31), rfx.reduce_reads_params(P=P)), P
    for kw in (dict(min_error_cov=0), dict(min_repeat_fold=0.5), dict(max_cov=-1), dict(min_cov=-1), dict(front_clip=-1), dict(end_clip=-1),
               dict(bubble=2), dict(sensitive=2), dict(min_cov=0), dict(min_cov=10001)):
        assert refused((23, 67) if kw == dict(min_cov=0) else (23, 31), rfx.reduce_reads_params(**kw)), kw
    assert refused((23, 31), None)
    assert refused((23, 31), ml=32 * store[2] + 1) and refused((23, 31), n_reads=-1)
    assert raw_call(rfx, store, len(reads), max_len, (23, 31), good, None) == E_ARG
    co = d._c()
    ks = (C.c_int * 2)(23, 31)
    per_k = (C.c_int64 * 2)()
    L, ctx, (dw, dn, wpr) = rfx.L, rfx.ctx, store
    assert L.rfx_dev_reduce_reads(ctx, None, dn.data_ptr(), len(reads), wpr, max_len, C.addressof(ks), 2, C.byref(good), C.byref(co), C.addressof(per_k)) == E_ARG
    assert L.rfx_dev_reduce_reads(ctx, dw.data_ptr(), None, len(reads), wpr, max_len, C.addressof(ks), 2, C.byref(good), C.byref(co), C.addressof(per_k)) == E_ARG
    assert L.rfx_dev_reduce_reads(ctx, dw.data_ptr(), dn.data_ptr(), len(reads), wpr, max_len, None, 2, C.byref(good), C.byref(co), C.addressof(per_k)) == E_ARG
    assert L.rfx_dev_reduce_reads(ctx, dw.data_ptr(), dn.data_ptr(), len(reads), wpr, max_len, C.addressof(ks), 2, C.byref(good), C.byref(co), None) == E_ARG
    assert untouched(d)


def test_the_text_form_with_a_short_buffer_reports_the_lengths_and_writes_nothing(rfx, synthetic):
    """rfx_reduce_text's rule: RFX_E_CAP with *out_len and every offset set, no byte written; with exactly the length it succeeds"""
    klist = (23, 31, 41)
    prm = rfx.reduce_reads_params(P=3)
    texts = rfx.reduce_reads_text([r.encode() for r in synthetic], klist, prm)
    need = sum(len(t) for t in texts)
    bases = np.frombuffer("".join(synthetic).encode(), np.uint8)
    off = np.zeros(len(synthetic) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in synthetic])
    ks = (C.c_int * 3)(*klist)
    for cap in (need - 1, 0, need):
        out, ln, offs = np.full(need + 16, FILL, np.uint8), C.c_int64(-77), np.full(4, -77, np.int64)
        st = rfx.L.rfx_reduce_reads(rfx.ctx, bases.ctypes.data, off.ctypes.data, len(synthetic), C.addressof(ks), 3, C.byref(prm), out.ctypes.data, cap,
                                    C.addressof(ln), offs.ctypes.data)
        assert st == (0 if cap == need else E_CAP) and ln.value == need
        assert offs.tolist() == [0, len(texts[0]), len(texts[0]) + len(texts[1]), need]
        assert (out[need:] == FILL).all() and ((out[:need].tobytes() == b"".join(texts)) if cap == need else (out == FILL).all())
    out, ln, offs = np.full(16, FILL, np.uint8), C.c_int64(-77), np.full(4, -77, np.int64)
    for bad in ((C.c_int * 3)(23, 31, 32), (C.c_int * 3)(31, 23, 41)):
        assert rfx.L.rfx_reduce_reads(rfx.ctx, bases.ctypes.data, off.ctypes.data, len(synthetic), C.addressof(bad), 3, C.byref(prm), out.ctypes.data, 16,
                                      C.addressof(ln), offs.ctypes.data) == E_ARG
    assert ln.value == -77 and (offs == -77).all() and (out == FILL).all()


def test_reflexiv_host_reduce_from_a_fastq_equals_counter_and_the_klist_mode(tmp_path):
    """`reflexiv_host reduce -fastq F -klist 23,31,41 -partition 8` against `counter` x 3 followed by `reduce -kmerc out -klist 23,31,41
    -partition 8`: the Count_*_reduced files byte for byte (no k of this list reaches 61, so the klist mode's missing E rule does not show)"""
    import subprocess
    exe = os.path.join(os.path.dirname(HERE), "reflexiv_amd", "reflexiv_host")
    fq = os.path.join(HERE, "golden", "paired_dat1.fq.gz")
    one, steps = tmp_path / "one", tmp_path / "steps"

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (args, r.stderr[-2000:])
    run("reduce", "-fastq", fq, "-klist", "23,31,41", "-partition", "8", "-outfile", str(one))
    for k in (23, 31, 41):
        run("counter", "-fastq", fq, "-kmer", str(k), "-outfile", str(steps))
    run("reduce", "-kmerc", str(steps), "-klist", "23,31,41", "-partition", "8", "-outfile", str(steps))
    for k in (23, 31, 41):
        a, b = (d / f"Count_{k}_reduced" / "part-00000.csv" for d in (one, steps))
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 1000, k
        assert (one / f"Count_{k}_reduced" / "_SUCCESS").exists()


def test_everything_again_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is 0xA5 before the library uses it.  A child process: the mask is read
    once per process"""
    import subprocess
    import sys
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
