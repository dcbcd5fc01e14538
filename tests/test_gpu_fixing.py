"""The contig fixing stage (Assembly_intermediate/04Fixing) on packed record sets in HBM (rfx_dev_fix_*, rfx_fix_text; DESIGN.md
section 19): every operator against its stage of the rows the reference's own classes made (tests/golden/fixing_vectors.npz),
unpacked field by field and as raw words against the numpy packer; every loop pass of the resident chain and the host form
against the stored passes and the final text; contig counts around the block size, runs of equal keys across a block edge for
both folds, partition starts on and past a block edge, 3,000-base contigs -- against the string model (tests/fixing_model.py,
which test_fixing_model.py pins to the same vectors); the argument, capacity and text-buffer contracts; the hand-over from the
dynamic-k iterations without a host copy; reflexiv_host fixing; and all of it again with every allocation poisoned."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import fixing_model as F
from tests.test_gpu_dynamic_edges import same_records
from tests.test_gpu_dynamic_packed import raw_equals, poisoned, untouched, FILL, OK, E_ARG, E_CAP, E_LIMIT
from tests.test_gpu_ksort import upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "fixing_vectors.npz")
MARK = (-30000, -7, -1, 0, 1, 2, 9, 30000)


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
    """every case, loaded once: name -> (params, P, rows, {stage: records}, {stage: part starts}, 31-mers, passes, text)"""
    z = np.load(VEC)
    return {n: F.load_case(z, n) for n in case_names()}


def cparams(rfx, p):
    return rfx.fix_params(p["max_k"], scramble=p["scramble"], max_iteration=p["max_iteration"])


def lines(rows):
    return [r if r.endswith("\n") else r + "\n" for r in rows]


def host(recs):
    """the model's records (key, marker, ext, left, right) -> DynRecords"""
    from reflexiv_amd.api import DynRecords
    return DynRecords.from_text([r[0] for r in recs], [r[2] for r in recs], [r[1] for r in recs], [r[3] for r in recs], [r[4] for r in recs])


def dev_starts(ps):
    import torch
    t = torch.tensor([int(x) for x in ps], dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    return t


def equals(rfx, pk, recs, tag):
    """the packed set in HBM is the record list: unpacked field by field, and word for word the numpy packer's (so every padding
    bit and every unused key word is 0)"""
    want = host(recs)
    same_records(rfx.dyn_unpack(pk), want, tag)
    raw_equals(pk, want, tag)


def value_of(kmer):
    """a 31-mer as rfx_dev_fix_contig_ends writes it: 62 bits, the first base in bits 61..60"""
    v = 0
    for ch in kmer:
        v = (v << 2) | "ACGT".index(ch)
    return v


def dev_values(kmers):
    import torch
    t = torch.from_numpy(np.array([value_of(k) for k in kmers] or [0], np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def rand_seq(rng, n):
    return "".join("ACGT"[b] for b in rng.integers(0, 4, n))


def text_of(rfx, pk):
    d_text, ln = rfx.dyn_to_text_dev(pk)
    return bytes(d_text[:ln].cpu().numpy()).decode()


def contig_rows(rng, n, mk, lo=0, hi=90):
    """n rows of an iteration's output: contigs of 2 max_k + lo .. 2 max_k + hi bases cut from one genome so that neighbours overlap
    and the loop merges them; both markers, every kind of left / right"""
    g = rand_seq(rng, 60 * n + 4 * mk + hi + 64)
    rows, pos = [], 0
    for _ in range(n):
        L = 2 * mk + int(rng.integers(lo, hi + 1))
        c = g[pos:pos + L]
        pos += int(rng.integers(20, 60))
        m = int(rng.integers(1, 3))
        kl = int(rng.choice((30, 31, 33, 64)))
        key, ext = (c[:kl], c[kl:]) if m == 1 else (c[L - kl:], c[:L - kl])
        rows.append(f"{key},{m}|{int(rng.choice(MARK))}|{int(rng.choice(MARK))},{ext}")
    return rows


def chain_equals_model(rfx, rows, p, P, tag):
    """the operators one by one on the device, each on the device's previous output, and the resident chain, against the model with
    the distinct 31-mers in the device's (ascending) order"""
    import torch
    want, wps, wk, wpasses = F.run_stages(rows, p, P, order="sorted")
    cp = cparams(rfx, p)
    d_text, d_off = upload(lines(rows))
    b = rfx.fix_binarize(d_text, d_off, cp)
    equals(rfx, b, want["binarized"], (tag, "binarized"))
    lg, d_k, nk = rfx.fix_contig_ends(b, cp)
    equals(rfx, lg, want["long"], (tag, "long"))
    assert nk == len(wk) and d_k[:nk].cpu().tolist() == [value_of(k) for k in wk], (tag, "31-mers")
    u = rfx.fix_kmer_set(d_k, nk, lg)
    equals(rfx, u, want["union"], (tag, "union"))
    s1, ps1 = rfx.dyn_sort_dev(u, P)
    equals(rfx, s1, want["sort1"], (tag, "sort1"))
    f1, ops1 = rfx.fix_fork_filter(s1, False, ps1)
    equals(rfx, f1, want["fold1"], (tag, "fold1"))
    r = rfx.fix_reflect(f1)
    equals(rfx, r, want["reflected"], (tag, "reflected"))
    s2, ps2 = rfx.dyn_sort_dev(r, P)
    equals(rfx, s2, want["sort2"], (tag, "sort2"))
    f2, ops2 = rfx.fix_fork_filter(s2, True, ps2)
    equals(rfx, f2, want["fold2"], (tag, "fold2"))
    assert (ps1.cpu().tolist(), ops1.cpu().tolist(), ps2.cpu().tolist(), ops2.cpu().tolist()) == (wps["sort1"], wps["fold1"], wps["sort2"], wps["fold2"]), tag
    out = rfx.fix_run(d_text, d_off, P, cp)
    equals(rfx, out, wpasses[-1], (tag, "run"))
    assert text_of(rfx, out) == F.to_text(wpasses[-1])
    assert rfx.fix_text("".join(lines(rows)).encode(), P, cp).decode() == F.to_text(wpasses[-1])
    torch.cuda.synchronize()
    return want, wpasses


# ---- 1. every operator against the reference's classes -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", case_names())
def test_every_operator_equals_its_stage_of_the_reference(rfx, vec, case):
    """each operator is fed the reference's previous output (packed by rfx_dev_dyn_pack) and the reference's partition starts; the
    sorts are rfx_dev_dyn_sort and the loop passes rfx_dev_dyn_extend_pass (stage 1, below iteration 61), both as they are"""
    p, P, rows, st, ps, kmers, passes, text = vec[case]
    cp = cparams(rfx, p)
    pk = lambda s: rfx.dyn_pack(host(st[s]))                                                # noqa: E731
    equals(rfx, rfx.fix_binarize(*upload(lines(rows)), cp), st["binarized"], (case, "binarized"))
    b = pk("binarized")
    lg, d_k, nk = rfx.fix_contig_ends(b, cp)
    equals(rfx, lg, st["long"], (case, "long"))
    assert nk == len(kmers) <= 2 * (p["max_k"] - 30) * b.n and d_k[:nk].cpu().tolist() == [value_of(k) for k in kmers], (case, "31-mers")
    u = rfx.fix_kmer_set(dev_values(kmers), len(kmers), pk("long"))
    equals(rfx, u, F.kmer_set(kmers, st["long"], "sorted"), (case, "union"))               # (the distinct set ascending: a stated deviation)
    assert sorted(F.kmer_set(kmers, st["long"], "sorted")) == sorted(st["union"])
    for src, dst in (("union", "sort1"), ("reflected", "sort2")):
        g, gps = rfx.dyn_sort_dev(pk(src), P)
        equals(rfx, g, st[dst], (case, dst))
        assert gps.cpu().tolist() == ps[dst], (case, dst, "partition starts")
    for src, dst, reflected in (("sort1", "fold1", False), ("sort2", "fold2", True)):
        d = pk(src)
        g, gps = rfx.fix_fork_filter(d, reflected, dev_starts(ps[src]))
        equals(rfx, g, st[dst], (case, dst))
        assert gps.cpu().tolist() == ps[dst] and g.n <= d.n and g.words <= d.words, (case, dst, "partition starts, capacity bound")
    equals(rfx, rfx.fix_reflect(pk("fold1")), st["reflected"], (case, "reflected"))
    # step 9 is the dynamic-k pass: once on the right fold's partitions, then behind a sort
    marker = 1 if p["scramble"] == 3 else 2
    cur, _ = rfx.dyn_extend_pass_dev(pk("fold2"), dev_starts(ps["fold2"]), stage=1, start_iteration=5, start_marker=marker)
    equals(rfx, cur, passes[0], (case, "pass", 0))
    for i in range(1, len(passes)):
        s, sps = rfx.dyn_sort_dev(cur, P)
        cur, _ = rfx.dyn_extend_pass_dev(s, sps, stage=1, start_iteration=5, start_marker=marker)
        equals(rfx, cur, passes[i], (case, "pass", i))
    assert text_of(rfx, cur) == text


@pytest.mark.parametrize("case", case_names())
def test_every_loop_pass_of_the_resident_chain_and_the_host_form(rfx, vec, case):
    """rfx_dev_fix_run with max_iteration = -1, 0, 1, ... stops behind every loop pass in turn: each against the stored pass; the
    case's own max_iteration against the final text, and rfx_fix_text too"""
    p, P, rows, st, ps, kmers, passes, text = vec[case]
    d_text, d_off = upload(lines(rows))
    for i in range(len(passes)):
        out = rfx.fix_run(d_text, d_off, P, cparams(rfx, dict(p, max_iteration=i - 1)))
        equals(rfx, out, passes[i], (case, "run to pass", i))
    out = rfx.fix_run(d_text, d_off, P, cparams(rfx, p))
    equals(rfx, out, passes[-1], (case, "run"))
    assert text_of(rfx, out) == text
    assert rfx.fix_text("".join(lines(rows)).encode(), P, cparams(rfx, p)).decode() == text
    assert rfx.last_call_ms > 0


# ---- 2. sizes, block edges, long contigs: against the model --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 3000])
def test_contig_counts_around_the_block_size(rfx, n):
    p = F.default_params(32, scramble=2 + n % 2, max_iteration=1)
    want, passes = chain_equals_model(rfx, contig_rows(np.random.default_rng(100 + n), n, 32), p, 3, n)
    assert len(want["binarized"]) == n and (n < 255 or len(passes[-1]) < len(want["fold2"]))


def test_a_duplicated_contig_makes_runs_of_equal_keys_through_the_whole_chain(rfx):
    """40 copies of one contig among 300 others: its long rows are a run of 40 equal keys in both folds, all kept in order"""
    rng = np.random.default_rng(5)
    rows = contig_rows(rng, 300, 31)
    rows[130:130] = [rows[7]] * 39
    want, _ = chain_equals_model(rfx, rows, F.default_params(31, max_iteration=0), 7, "duplicates")
    from collections import Counter
    assert max(Counter(r[0] for r in want["sort1"] if len(r[2]) > 1).values()) >= 40


@pytest.mark.parametrize("reflected", [False, True])
@pytest.mark.parametrize("kind", ["ones", "ones then longs", "mixed", "ties"])
def test_a_run_of_equal_keys_across_a_block_edge(rfx, reflected, kind):
    """600 sorted keys of one row each and one run of 24 rows put on rows 245..268, across the edge at 256: one-base rows only (the
    LAST row of the smallest code survives), one-base rows ahead of longer ones, the two mixed (the driver never makes that for
    the left fold), and ties of the smallest code.  P = 1, and cuts on and one past the block edge, inside the run"""
    rng = np.random.default_rng(17 + len(kind))
    keys = sorted({rand_seq(rng, 30) for _ in range(640)}, key=lambda k: F.pm.dyn_blocks(k))[:601]
    m = 2 if reflected else 1
    one = lambda key, ch, j: (key, m, ch, -1 - j, j)                 # noqa: E731
    lng = lambda key, j: (key, m, rand_seq(rng, 2 + 31 * (j % 4)), j, -j)                  # noqa: E731
    recs = [one(k, "ACGT"[int(rng.integers(0, 4))], i) if i % 3 else lng(k, i) for i, k in enumerate(keys)]
    K = keys[245]
    if kind == "ones":
        run = [one(K, "GCTGTCGG"[j % 8], j) for j in range(24)]
    elif kind == "ones then longs":
        run = [one(K, "ACGT"[j % 4], j) for j in range(14)] + [lng(K, j) for j in range(10)]
    elif kind == "mixed":
        run = [lng(K, j) if j in (3, 11, 12, 23) else one(K, "ACGT"[j % 4], j) for j in range(24)]
    else:
        run = [one(K, "TCGC"[j % 4], j) for j in range(24)]
    recs[245:246] = run
    n = len(recs)
    d = rfx.dyn_pack(host(recs))
    for ps in ([0, n], [0, 256, n], [0, 100, 257, 257, n], [0, 245, 256, 257, 269, n]):
        want, _, wps = F.by_partition(F.fold, recs, len(ps) - 1, ps)
        assert want == F.by_partition(F.fold_closed_form, recs, len(ps) - 1, ps)[0]
        g, gps = rfx.fix_fork_filter(d, reflected, dev_starts(ps))
        equals(rfx, g, want, (kind, reflected, ps))
        assert gps.cpu().tolist() == wps
        if len(ps) == 2:
            assert len(want) == n - 24 + {"ones": 1, "ones then longs": 10, "mixed": 4, "ties": 1}[kind]
    # 63 partitions of one row each at the front: every row is a partition's first, nothing is compared
    ps = list(range(63)) + [n]
    want, _, wps = F.by_partition(F.fold, recs, 63, ps)
    g, gps = rfx.fix_fork_filter(d, reflected, dev_starts(ps))
    equals(rfx, g, want, (kind, reflected, "63 partitions"))
    assert gps.cpu().tolist() == wps and want[:62] == recs[:62]


@pytest.mark.parametrize("mk", [31, 64, 124])
def test_3000_base_contigs_span_many_words(rfx, mk):
    """contigs of 3,000..3,130 bases under both markers and keys of 30..124 bases: the trimmed copy's ~94 words, the reflection's, and
    the 31-mers cut across the key / extension seam and across word edges"""
    rng = np.random.default_rng(mk)
    recs = []
    for j in range(24):
        c = rand_seq(rng, 3000 + 5 * j + (j % 3))
        kl = (30, 31, 32, 33, 63, 64, 65, 95, 96, 97, 123, 124)[j % 12]
        m = 1 + j % 2
        key, ext = (c[:kl], c[kl:]) if m == 1 else (c[len(c) - kl:], c[:len(c) - kl])
        recs.append((key, m, ext, int(rng.choice(MARK)), int(rng.choice(MARK))))
    recs.insert(5, (rand_seq(rng, 40), 1, rand_seq(rng, 2 * mk - 41), 3, 3))                # one short of 2 max_k: nothing
    p = F.default_params(mk)
    longs, kmers = F.contig_ends(recs, p)
    assert len(longs) == 24
    lg, d_k, nk = rfx.fix_contig_ends(rfx.dyn_pack(host(recs)), cparams(rfx, p))
    equals(rfx, lg, longs, (mk, "long"))
    assert nk == len(kmers) == 24 * 2 * (mk - 30) and d_k[:nk].cpu().tolist() == [value_of(k) for k in kmers]
    equals(rfx, rfx.fix_reflect(lg), F.reflect(longs), (mk, "reflected"))
    equals(rfx, rfx.fix_reflect(rfx.fix_reflect(lg)), F.reflect(longs), (mk, "reflected twice: a reflected record stays"))


# ---- 3. contracts --------------------------------------------------------------------------------------------------------------------
def thunks(rfx, vec):
    """every entry point with a packed output, as thunks (params, output struct, P) -> status, on the stages of k41_P7_s2_M3"""
    import torch
    p, P, rows, st, ps, kmers, passes, text = vec["k41_P7_s2_M3"]
    L, ctx = rfx.L, rfx.ctx
    dt = upload(lines(rows))
    sets = {s: rfx.dyn_pack(host(st[s])) for s in ("binarized", "long", "sort1", "fold1", "sort2")}
    ci = {s: d._c() for s, d in sets.items()}
    starts = {s: dev_starts(ps[s]) for s in ("sort1", "sort2")}
    vals = dev_values(kmers)
    ops_out = torch.full((65,), -77, dtype=torch.int64, device="cuda")
    kmers_out = torch.full((len(kmers) + 8,), -77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nk = C.c_int64(-77)
    keep = (dt, sets, ci, starts, vals, ops_out, kmers_out, nk)
    txt = (dt[0].data_ptr(), dt[1].data_ptr(), len(rows))
    ops = {
        "binarize": lambda cp, co, P=P: L.rfx_dev_fix_binarize(ctx, *txt, C.byref(cp), C.byref(co)),
        "contig_ends": lambda cp, co, P=P: L.rfx_dev_fix_contig_ends(ctx, C.byref(ci["binarized"]), C.byref(cp), C.byref(co), kmers_out.data_ptr(),
                                                                     int(kmers_out.numel()), C.addressof(nk)),
        "kmer_set": lambda cp, co, P=P: L.rfx_dev_fix_kmer_set(ctx, vals.data_ptr(), len(kmers), C.byref(ci["long"]), C.byref(co)),
        "fork_filter 0": lambda cp, co, P=P: L.rfx_dev_fix_fork_filter(ctx, 0, C.byref(ci["sort1"]), starts["sort1"].data_ptr(), P, C.byref(co), ops_out.data_ptr()),
        "reflect": lambda cp, co, P=P: L.rfx_dev_fix_reflect(ctx, C.byref(ci["fold1"]), C.byref(co)),
        "fork_filter 1": lambda cp, co, P=P: L.rfx_dev_fix_fork_filter(ctx, 1, C.byref(ci["sort2"]), starts["sort2"].data_ptr(), P, C.byref(co), ops_out.data_ptr()),
        "run": lambda cp, co, P=P: L.rfx_dev_fix_run(ctx, *txt, P, C.byref(cp), C.byref(co)),
    }
    return p, P, rows, ops, keep


@pytest.mark.parametrize("mk", [30, 125, 0, -5])
def test_a_refused_max_k_returns_the_code_and_writes_nothing(rfx, vec, mk):
    p, P, rows, ops, keep = thunks(rfx, vec)
    cp = rfx.fix_params(mk)
    for name in ("binarize", "contig_ends", "run"):
        d = poisoned(4000, 4000)
        co = d._c()
        co.n = co.need_words = -77
        assert ops[name](cp, co) == E_ARG, (name, mk)
        assert untouched(d) and (int(co.n), int(co.need_words)) == (-77, -77), (name, mk)
    assert keep[7].value == -77 and bool((keep[6] == -77).all())
    assert ops["run"](rfx.fix_params(41, max_iteration=-2), poisoned(8, 8)._c()) == E_ARG
    o, ln = np.full(64, FILL, np.uint8), C.c_int64(-77)
    off = np.array([0, 8], np.int64)
    assert rfx.L.rfx_fix_text(rfx.ctx, b"A,1|2|3,", off.ctypes.data, 1, 1, C.byref(cp), o.ctypes.data, 64, C.addressof(ln)) == E_ARG
    assert ln.value == -77 and (o == FILL).all()


def test_bad_partition_counts_null_pointers_bad_starts_and_keys_that_are_not_30_bases(rfx, vec):
    p, P, rows, ops, keep = thunks(rfx, vec)
    cp = cparams(rfx, p)
    dt, sets, ci, starts, vals, ops_out, kmers_out, nk = keep
    L, ctx = rfx.L, rfx.ctx
    d = poisoned(20000, 20000)
    for bad_p in (0, 64, -1):
        for name in ("fork_filter 0", "fork_filter 1", "run"):
            assert ops[name](cp, d._c(), bad_p) == E_ARG, (name, bad_p)
    o, ln = np.full(64, FILL, np.uint8), C.c_int64(-77)
    off = np.array([0, 8], np.int64)
    for bad_p in (0, 64):
        assert L.rfx_fix_text(ctx, b"A,1|2|3,", off.ctypes.data, 1, bad_p, C.byref(cp), o.ctypes.data, 64, C.addressof(ln)) == E_ARG
    # null pointers
    txt = (dt[0].data_ptr(), dt[1].data_ptr(), len(rows))
    assert L.rfx_dev_fix_binarize(ctx, None, txt[1], txt[2], C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix_binarize(ctx, txt[0], None, txt[2], C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix_binarize(ctx, *txt, None, C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix_binarize(ctx, *txt, C.byref(cp), None) == E_ARG
    assert L.rfx_dev_fix_run(ctx, *txt, P, None, C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix_run(ctx, *txt, P, C.byref(cp), None) == E_ARG
    assert L.rfx_dev_fix_contig_ends(ctx, None, C.byref(cp), C.byref(d._c()), kmers_out.data_ptr(), 8, C.addressof(nk)) == E_ARG
    assert L.rfx_dev_fix_contig_ends(ctx, C.byref(ci["binarized"]), C.byref(cp), C.byref(d._c()), None, 8, C.addressof(nk)) == E_ARG
    assert L.rfx_dev_fix_contig_ends(ctx, C.byref(ci["binarized"]), C.byref(cp), C.byref(d._c()), kmers_out.data_ptr(), 8, None) == E_ARG
    assert L.rfx_dev_fix_kmer_set(ctx, None, 5, C.byref(ci["long"]), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix_kmer_set(ctx, vals.data_ptr(), 5, None, C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix_fork_filter(ctx, 0, C.byref(ci["sort1"]), None, P, C.byref(d._c()), ops_out.data_ptr()) == E_ARG
    assert L.rfx_dev_fix_fork_filter(ctx, 0, C.byref(ci["sort1"]), starts["sort1"].data_ptr(), P, C.byref(d._c()), None) == E_ARG
    assert L.rfx_dev_fix_fork_filter(ctx, 2, C.byref(ci["sort1"]), starts["sort1"].data_ptr(), P, C.byref(d._c()), ops_out.data_ptr()) == E_ARG
    assert L.rfx_dev_fix_reflect(ctx, None, C.byref(d._c())) == E_ARG
    no_key = d._c()
    no_key.key = None
    assert L.rfx_dev_fix_reflect(ctx, C.byref(ci["fold1"]), C.byref(no_key)) == E_ARG
    # partition starts that do not run from 0 to n
    m = sets["sort1"].n
    for bad in ([1, m], [0, m - 1], [0, m + 1], [0, 9, 5, m], [0, -3, m], [0, m + 5, m]):
        t = dev_starts(bad)
        assert L.rfx_dev_fix_fork_filter(ctx, 0, C.byref(ci["sort1"]), t.data_ptr(), len(bad) - 1, C.byref(d._c()), ops_out.data_ptr()) == E_ARG, bad
    # a key that is not 30 bases where the operator expects one; a record without an extension
    rng = np.random.default_rng(2)
    rec = lambda kl, el: (rand_seq(rng, kl), 1, rand_seq(rng, el), 3, 3)                     # noqa: E731
    t2 = dev_starts([0, 2])
    for recs in ([rec(30, 5), rec(31, 5)], [rec(29, 1), rec(30, 1)], [rec(30, 0), rec(30, 4)]):
        c = rfx.dyn_pack(host(recs))._c()
        assert L.rfx_dev_fix_fork_filter(ctx, 0, C.byref(c), t2.data_ptr(), 1, C.byref(d._c()), ops_out.data_ptr()) == E_ARG
        assert L.rfx_dev_fix_fork_filter(ctx, 1, C.byref(c), t2.data_ptr(), 1, C.byref(d._c()), ops_out.data_ptr()) == E_ARG
        assert L.rfx_dev_fix_reflect(ctx, C.byref(c), C.byref(d._c())) == E_ARG
        assert L.rfx_dev_fix_kmer_set(ctx, vals.data_ptr(), 5, C.byref(c), C.byref(d._c())) == E_ARG
    # a 31-mer value of 2^62 or more; partition starts that do not run from 0 to 0 on an empty set
    big_val = dev_values(["A" * 31, "C" * 31])
    big_val[1] = 1 << 62
    import torch
    torch.cuda.synchronize()
    assert L.rfx_dev_fix_kmer_set(ctx, big_val.data_ptr(), 2, C.byref(ci["long"]), C.byref(d._c())) == E_ARG
    empty = rfx.fix_binarize(*upload([]), cp)._c()
    for bad in ([0, 1], [1, 0], [0, 2, 0]):
        t = dev_starts(bad)
        assert L.rfx_dev_fix_fork_filter(ctx, 1, C.byref(empty), t.data_ptr(), len(bad) - 1, C.byref(d._c()), ops_out.data_ptr()) == E_ARG, bad
    assert L.rfx_dev_fix_fork_filter(ctx, 1, C.byref(empty), dev_starts([0, 0, 0]).data_ptr(), 2, C.byref(poisoned(4, 4)._c()), ops_out.data_ptr()) == OK
    ops_out.fill_(-77)
    # the stated deviation: a sub-k-mer of more than 124 bases is RFX_E_LIMIT for the set
    for ext in (200, 1):
        bad_rows = upload(lines(rows[:3]) + [f"{rand_seq(rng, 125)},1|2|3,{rand_seq(rng, ext)}\n"])
        assert L.rfx_dev_fix_binarize(ctx, bad_rows[0].data_ptr(), bad_rows[1].data_ptr(), 4, C.byref(cp), C.byref(d._c())) == E_LIMIT
        assert L.rfx_dev_fix_run(ctx, bad_rows[0].data_ptr(), bad_rows[1].data_ptr(), 4, P, C.byref(cp), C.byref(d._c())) == E_LIMIT
    assert untouched(d) and bool((ops_out == -77).all()) and bool((kmers_out == -77).all()) and nk.value == -77
    assert ln.value == -77 and (o == FILL).all()


def test_every_capacity_one_short(rfx, vec):
    """cap_n = need - 1, then cap_words = need - 1, and for the contig ends cap_kmers = need - 1: RFX_E_CAP with n / need_words /
    *n_kmers set, every output tensor (0xA5), the 31-mer array and the output partition starts as they were; with exactly the needs
    the same call succeeds.  The needs stay within the capacities the header states"""
    p, P, rows, ops, keep = thunks(rfx, vec)
    dt, sets, ci, starts, vals, ops_out, kmers_out, nk = keep
    cp = cparams(rfx, p)
    n, nbytes, cut2 = len(rows), int(dt[0].numel()), 2 * (p["max_k"] - 30)
    bound = {"binarize": (n, n + nbytes // 32), "contig_ends": (sets["binarized"].n, sets["binarized"].words + 4 * sets["binarized"].n),
             "kmer_set": (len(keep[4]) + sets["long"].n, len(keep[4]) + sets["long"].words), "fork_filter 0": (sets["sort1"].n, sets["sort1"].words),
             "reflect": (sets["fold1"].n, sets["fold1"].words), "fork_filter 1": (sets["sort2"].n, sets["sort2"].words),
             "run": (n * (cut2 + 1), n * (cut2 + 1) + nbytes // 32)}
    for name, call in ops.items():
        big = poisoned(20000, 20000)
        co = big._c()
        assert call(cp, co) == OK, name
        need_n, need_w = int(co.n), int(co.need_words)
        assert 0 < need_n <= bound[name][0] and 0 < need_w <= bound[name][1], (name, need_n, need_w, bound[name])
        exact = poisoned(need_n, need_w)
        assert call(cp, exact._c()) == OK and not untouched(exact), name
        ops_out.fill_(-77)
        kmers_out.fill_(-77)
        for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
            d = poisoned(cap_n, cap_w)
            co = d._c()
            co.n = co.need_words = -77
            assert call(cp, co) == E_CAP, (name, cap_n, cap_w)
            assert (int(co.n), int(co.need_words)) == (need_n, need_w), name
            assert untouched(d) and bool((ops_out == -77).all()) and bool((kmers_out == -77).all()), (name, cap_n, cap_w)
    need_k = nk.value
    assert need_k == len(vals) <= cut2 * sets["binarized"].n
    d = poisoned(20000, 20000)
    co = d._c()
    co.n = co.need_words = -77
    got = C.c_int64(-77)
    assert rfx.L.rfx_dev_fix_contig_ends(rfx.ctx, C.byref(ci["binarized"]), C.byref(cp), C.byref(co), kmers_out.data_ptr(), need_k - 1, C.addressof(got)) == E_CAP
    assert got.value == need_k and int(co.n) == sets["long"].n and untouched(d) and bool((kmers_out == -77).all())


def test_the_text_buffer_one_byte_short(rfx, vec):
    p, P, rows, st, ps, kmers, passes, text = vec["k41_P7_s2_M3"]
    cp = cparams(rfx, p)
    t = "".join(lines(rows)).encode()
    off, n = rfx._row_offsets(t)
    for cap in (len(text) - 1, 0):
        o, ln = np.full(len(text) + 16, FILL, np.uint8), C.c_int64(0)
        assert rfx.L.rfx_fix_text(rfx.ctx, t, off.ctypes.data, n, P, C.byref(cp), o.ctypes.data, cap, C.addressof(ln)) == E_CAP
        assert ln.value == len(text) and (o == FILL).all()
    o, ln = np.full(len(text) + 16, FILL, np.uint8), C.c_int64(0)
    assert rfx.L.rfx_fix_text(rfx.ctx, t, off.ctypes.data, n, P, C.byref(cp), o.ctypes.data, len(text), C.addressof(ln)) == OK
    assert o[:len(text)].tobytes().decode() == text and (o[len(text):] == FILL).all()


def test_an_empty_input_through_every_entry_point(rfx):
    cp = rfx.fix_params(41)
    none, short = upload([]), upload(["ACGTACGT,1|2|3,ACGT\n"])       # (a row below 2 max_k: dropped)
    b = rfx.fix_binarize(*none, cp)
    lg, d_k, nk = rfx.fix_contig_ends(b, cp)
    u = rfx.fix_kmer_set(d_k, nk, lg)
    s, ps = rfx.dyn_sort_dev(u, 5)
    f0, ps0 = rfx.fix_fork_filter(s, False, ps)
    f1, ps1 = rfx.fix_fork_filter(s, True, ps)
    outs = [b, lg, u, f0, f1, rfx.fix_reflect(f0), rfx.fix_run(*none, 5, cp), rfx.fix_run(*short, 1, cp), rfx.fix_binarize(*short, cp)]
    for t in outs:
        assert t.n == 0 and int(t.ext_off[0]) == 0
    assert nk == 0 and ps0.cpu().tolist() == [0] * 6 == ps1.cpu().tolist()
    assert rfx.fix_text(b"", 3, cp) == b"" and rfx.fix_text(b"ACGTACGT,1|2|3,ACGT\n", 3, cp) == b""
    # 31-mers without long records, long records without 31-mers
    rng = np.random.default_rng(4)
    km = [rand_seq(rng, 31) for _ in range(5)]
    equals(rfx, rfx.fix_kmer_set(dev_values(km + km[:2]), 7, lg), F.kmer_set(km, [], "sorted"), "31-mers only")
    longs = [(rand_seq(rng, 30), 1, rand_seq(rng, 70), 1, -1)]
    equals(rfx, rfx.fix_kmer_set(d_k, 0, rfx.dyn_pack(host(longs))), longs, "long records only")


# ---- 4. the hand-over and the host program -------------------------------------------------------------------------------------------
def test_the_iterations_hand_their_text_to_the_stage_without_a_host_copy(rfx):
    """rfx_dev_dyn_run (thirty iterations of case c4 of tests/golden/dynamic_vectors.npz) -> rfx_dev_dyn_to_text -> the row offsets
    from the newlines, on the device -> rfx_dev_fix_run; the text is copied back only to give the model the same rows"""
    import torch
    z = np.load(os.path.join(ROOT, "tests", "golden", "dynamic_vectors.npz"))
    P, start, end = (int(x) for x in z["c4/meta"])
    rows = z["c4/it_binarized"].tobytes().decode().splitlines(True)
    it = rfx.dyn_binarize_dev(*upload(rows), 1)
    out, trace = rfx.dyn_run_dev(it, P=P, start_iteration=start, end_iteration=end)
    d_text, ln = rfx.dyn_to_text_dev(out)
    ends = torch.nonzero(d_text[:ln] == 10).flatten() + 1
    d_off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), ends.to(torch.int64)])
    torch.cuda.synchronize()
    assert int(d_off.numel()) == out.n + 1
    p = F.default_params(31, max_iteration=2)
    fixed = rfx.fix_run(d_text[:ln], d_off, 2, cparams(rfx, p))
    text = bytes(d_text[:ln].cpu().numpy()).decode()
    assert text == z["c4/final"].tobytes().decode()
    st, _, _, passes = F.run_stages(text.splitlines(), p, 2, order="sorted")
    assert len(st["binarized"]) > 0 and len(passes[-1]) < len(st["fold2"])
    equals(rfx, fixed, passes[-1], "hand-over")
    assert text_of(rfx, fixed) == F.to_text(passes[-1])


@pytest.mark.parametrize("case", ["k41_P7_s2_M3", "k31_P7_s3_M0"])
def test_reflexiv_host_fixing_writes_04Fixing(vec, tmp_path, case):
    import subprocess
    p, P, rows, st, ps, kmers, passes, text = vec[case]
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    src, out = tmp_path / "part-00000.csv", tmp_path / "out"
    src.write_text("".join(lines(rows)))
    r = subprocess.run([exe, "fixing", "-kmerc", str(src), "-klist", f"23,{p['max_k']}", "-partition", str(P), "-maxiter", str(p["max_iteration"]),
                        "-scramble", str(p["scramble"]), "-outfile", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = out / "Assembly_intermediate" / "04Fixing"
    assert (d / "part-00000.csv").read_text() == text and (d / "_SUCCESS").exists()


# ---- 5. poisoned allocations ---------------------------------------------------------------------------------------------------------
def test_the_stage_holds_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it, so a producer that
    relied on zeroed memory for its padding bits or unused key words fails the raw-word checks above.  A child process: the mask is
    read once per process."""
    import subprocess
    import sys
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
