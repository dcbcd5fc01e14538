"""The contig extension stages (Assembly_intermediate/08Extend and 09ExtendAgain) on packed sets in HBM (rfx_dev_ext_*, rfx_ext_text,
rfx_dev_ext2_to_text, rfx_ext2_text): every entry point against its stage of the rows the reference's own
classes made (tests/golden/extend_vectors.npz) -- sets unpacked and as raw words, from the text and from the device's form with the
literals in flags --; the chains on the device with no text in between, from rfx_dev_endext_contigs to the set rfx_dev_dedup_contigs
takes; both reflexiv_host subcommands against the stored texts; the smallest shapes that can go wrong against the string model
(tests/extend_model.py, which test_extend_model.py pins to the same vectors); the text-buffer rule at any alignment of the
destination; the argument, capacity and limit contracts; and all of it again with every allocation poisoned."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import endext_model as E
from tests import extend_model as X
from tests import fixing2_model as F2
from tests.test_gpu_dynamic_packed import poisoned, untouched, FILL, OK, E_ARG, E_CAP, E_LIMIT
from tests.test_gpu_endext import packed_equals, dev_contigs, rows_up
from tests.test_gpu_fixing import cparams, equals, lines, rand_seq, text_of, value_of
from tests.test_gpu_ksort import upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = (-30000, -7, -1, 0, 1, 2, 9, 30000)


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


@pytest.fixture(scope="module")
def vec():
    """every case, loaded once: name -> (params, P, rows, {stage: records}, {stage: part starts}, 31-mers, passes, text, rounds of 09,
    text of 09)"""
    z = np.load(X.VEC)
    return {n: X.load_case(z, n) for n in X.case_names()}


def dev_set(rfx, cs):
    """the model's device view [{bases, left, ...}] -> an EndextSet in HBM, as rfx_dev_endext_contigs leaves one"""
    import torch
    from reflexiv_amd.api import EndextSet
    s = EndextSet(len(cs), 1)
    s.set = rfx.contigs_pack([c["bases"] for c in cs])
    for a in s.ARRAYS:
        setattr(s, a, torch.from_numpy(np.array([c[a] for c in cs] or [0], np.int32)).cuda())
    torch.cuda.synchronize()
    return s


def set_equals(rfx, s, cs, tag):
    packed_equals(rfx, s.set, [c["bases"] for c in cs], (tag, "bases"))
    got = s.host()
    for a in s.ARRAYS:
        assert got[a].tolist() == [c[a] for c in cs], (tag, a)


def ends_equal(rfx, s, prm, longs, kmers, tag):
    lg, d_k, nk = rfx.ext_contig_ends(s, prm)
    equals(rfx, lg, longs, (tag, "long"))
    assert nk == len(kmers) and d_k[:nk].cpu().tolist() == [value_of(k) for k in kmers], (tag, "31-mers")
    assert nk <= 606 * max(s.n, 1) and lg.words <= s.set.words
    return lg


def text2_of(rfx, c):
    t, n = rfx.ext2_to_text(c)
    return bytes(t[:n].cpu().numpy()).decode()


def stage_equals_model(rfx, rows, p, P, tag):
    """both views of one input through every entry point of 08, against the string model with the distinct 31-mers in the device's
    (ascending) order -> (the text of 08, the set behind the run)"""
    want, wps, wk, wpasses = X.run_stages(rows, p, P, order="sorted")
    prm = cparams(rfx, p)
    s_text = rfx.ext_from_text(*upload(lines(rows)), prm)
    set_equals(rfx, s_text, X.device_set(rows, p, False), (tag, "from text"))
    assert rfx.last_call_ms > 0
    s_dev = dev_set(rfx, X.device_set(rows, p, True))
    text = X.to_text(wpasses[-1])
    out = None
    for view, s in (("text", s_text), ("flags", s_dev)):
        ends_equal(rfx, s, prm, want["long"], wk, (tag, view))
        out = rfx.ext_run(s, P, prm)
        equals(rfx, out, wpasses[-1], (tag, view, "run"))
        assert text_of(rfx, out) == text, (tag, view)
    assert rfx.ext_text("".join(lines(rows)).encode(), P, prm).decode() == text, (tag, "host form")
    return text, out


def stage2_equals_model(rfx, text, p, P, tag, resident=None):
    """09 on the text of 08 (and on the resident set of 08, with no text in between) against the string model -> the contig set"""
    prm = cparams(rfx, p)
    recs, rounds, cs, text2 = X.run2_stages(text.splitlines(), p, P)
    c = None
    for src in ([rfx.fix2_binarize(*upload(lines(text.splitlines())))] if text else []) + ([resident] if resident is not None else []):
        c, dl, dr = rfx.fix2_contigs(rfx.fix2_run(src, P, prm), prm)
        packed_equals(rfx, c, [x[0] for x in cs], (tag, "contigs"))
        assert text2_of(rfx, c) == text2, tag
    assert rfx.ext2_text(text.encode(), P, prm).decode() == text2, (tag, "host form")
    return c, text2


# ---- 1. every entry point against the reference's classes ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.case_names())
def test_every_entry_point_equals_its_stage_of_the_reference(rfx, vec, case):
    p, P, rows, st, ps, kmers, passes, text, rounds2, text2 = vec[case]
    prm = cparams(rfx, p)
    s = rfx.ext_from_text(*upload(lines(rows)), prm)
    assert [X.set_text_chars(c) for c in X.device_set(rows, p, False)] == [r[0] + r[2] for r in st["binarized"]]
    set_equals(rfx, s, X.device_set(rows, p, False), case)
    ends_equal(rfx, s, prm, st["long"], kmers, (case, "text"))
    ends_equal(rfx, dev_set(rfx, X.device_set(rows, p, True)), prm, st["long"], kmers, (case, "flags"))
    first = rfx.ext_run(s, P, cparams(rfx, dict(p, max_iteration=-1)))                     # the unsorted first pass only
    equals(rfx, first, passes[0], (case, "pass 0"))
    out = rfx.ext_run(dev_set(rfx, X.device_set(rows, p, True)), P, prm)
    equals(rfx, out, passes[-1], (case, "run"))
    assert text_of(rfx, out) == text == rfx.ext_text("".join(lines(rows)).encode(), P, prm).decode()
    # 09: the first round, every round, the contigs and the text; the resident set of 08 gives the same
    b = rfx.fix2_binarize(*upload(lines(text.splitlines())))
    if rounds2:
        equals(rfx, rfx.fix2_run(b, P, cparams(rfx, dict(p, max_iteration=0))), rounds2[0][2], (case, "09 round 0"))
        equals(rfx, rfx.fix2_run(out, P, prm), rounds2[-1][2], (case, "09 rounds, resident"))
    c, got2 = stage2_equals_model(rfx, text, p, P, case, resident=out)
    assert got2 == text2
    d, _ = rfx.dedup_dev(c)                                          # what rfx_dev_dedup_contigs takes
    assert 0 < d.n <= c.n


def test_endext_contigs_feed_the_stage_with_no_text_in_between(rfx):
    """rfx_dev_endext_contigs -> rfx_dev_ext_run -> rfx_dev_dyn_to_text equals 07EndExtend's text -> rfx_ext_text, and on through 09"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "endext_vectors.npz"))
    flagged = 0
    for case, P in (("crafted_k31", 2), ("fix_fix_k41_P7_s2_M3", 7)):
        mk, ctext, row_lines, cons, spliced, text07 = E.load_case(z, case)
        p = X.default_params(mk, max_iteration=3)
        prm = cparams(rfx, p)
        c, dl, dr = dev_contigs(rfx, E.contigs_of_text(ctext))
        s = rfx.endext_contigs(c, dl, dr, rfx.endext_consensus(c, dl, dr, *rows_up(row_lines)), mk)
        flagged += int(s.flags[:s.n].cpu().numpy().astype(bool).sum())
        out = rfx.ext_run(s, P, prm)
        text = text_of(rfx, out)
        assert text == rfx.ext_text(text07.encode(), P, prm).decode() == X.run_text(text07.splitlines(), p, P), case
        stage2_equals_model(rfx, text, p, P, case, resident=out)
    assert flagged >= 8                                              # flagged seams on the way: the literals never were text


@pytest.mark.parametrize("case", ("k41_P7_s2_M3", "k99_P2_s2_M3"))
def test_reflexiv_host_writes_the_stored_texts(vec, tmp_path, case):
    p, P, rows, st, ps, kmers, passes, text, rounds2, text2 = vec[case]
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    d = tmp_path / "07EndExtend"
    d.mkdir()
    (d / "part-00000.csv").write_text("".join(lines(rows)))
    out = tmp_path / "out"
    common = ["-klist", f"23,{p['max_k']}", "-partition", str(P), "-maxiter", str(p["max_iteration"]), "-scramble", str(p["scramble"]), "-outfile", str(out)]
    r = subprocess.run([exe, "extend", "-kmerc", str(d)] + common, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d8 = out / "Assembly_intermediate" / "08Extend"
    assert (d8 / "part-00000.csv").read_text() == text and (d8 / "_SUCCESS").exists()
    r = subprocess.run([exe, "extend2", "-kmerc", str(d8)] + common, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d9 = out / "Assembly_intermediate" / "09ExtendAgain"
    assert (d9 / "part-00000.csv").read_text() == text2 and (d9 / "_SUCCESS").exists()


# ---- 2. the smallest shapes that can go wrong, against the string model ---------------------------------------------------------------
def end_row(rng, idx, L, ll, rl, fl=False, fr=False, left=None, right=None, contig=None, le=None, re=None):
    """a row of 07EndExtend: ends of ll / rl BASES, the literals behind the left end and ahead of the right one where flagged"""
    contig = contig or rand_seq(rng, L)
    lt = (rand_seq(rng, ll) if le is None else le) + ("-1l" if fl else "")
    rt = ("r1-" if fr else "") + (rand_seq(rng, rl) if re is None else re)
    left = int(rng.choice(MARK)) if left is None else left
    right = int(rng.choice(MARK)) if right is None else right
    return f">Contig_{len(contig)}_{left}_{right}_{idx}_{len(lt)}_{len(rt)}_{idx},{lt}{contig}{rt}"


def genome_rows(rng, n, mk):
    """n contigs cut from one genome with the ends that reach into their neighbours: the loop joins them"""
    g = rand_seq(rng, 150 * n + 4 * mk + 800)
    rows, pos = [], 310
    for i in range(n):
        L = 2 * mk + int(rng.integers(0, 60))
        ll, rl = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        rows.append(end_row(rng, i, L, ll, rl, fl=i % 5 == 1, fr=i % 7 == 2, contig=g[pos:pos + L], le=g[pos - ll:pos], re=g[pos + L:pos + L + rl]))
        pos += L + int(rng.integers(-20, 40))
    return rows


@pytest.mark.parametrize("n", (0, 1, 2, 255, 256, 257))
def test_contig_counts_around_a_block(rfx, n):
    rng = np.random.default_rng(200 + n)
    p = X.default_params(31, max_iteration=2)
    rows = genome_rows(rng, n, 31)
    text, out = stage_equals_model(rfx, rows, p, 3, n)
    assert (text == "") == (n == 0)
    stage2_equals_model(rfx, text, p, 3, n, resident=out)


def test_one_contig_whose_end_kmers_cross_a_block(rfx):
    rng = np.random.default_rng(11)
    p = X.default_params(31, max_iteration=0)
    rows = [end_row(rng, 0, 90, 300, 300, True, True), end_row(rng, 1, 70, 300, 0, True, False), end_row(rng, 2, 64, 0, 300, False, True)]
    dev = X.device_set(rows, p)
    assert dev[0]["left_len"] + dev[0]["right_len"] == 606
    stage_equals_model(rfx, rows, p, 1, "606")


def test_the_cut_offset_at_every_residue_and_the_seam_at_every_window_offset(rfx):
    """left ends of 0..34 bases under each flag pattern: the cut contig starts at every residue mod 32 of the words, and the windows
    slide over both seams, so a seam lies at every offset 0..30 of some window and overlaps it by 1, 2 and 3 characters"""
    rng = np.random.default_rng(12)
    p = X.default_params(31, max_iteration=0)
    rows = []
    for f in range(4):
        for e in range(35):
            rows.append(end_row(rng, len(rows), 62 + (e * 7) % 40, e, (e * 5) % 36, bool(f & 1), bool(f & 2)))
    dev = X.device_set(rows, p)
    for f in range(4):
        assert {(c["left_len"] - 3 * (c["flags"] & 1)) % 32 for c in dev if c["flags"] == f} == set(range(32)), f
    assert X.seam_overlaps(dev, p) == {(s, n) for s in "LR" for n in (1, 2, 3)}
    offs = set()
    for c in dev:                                                    # where a seam begins inside a window
        T = len(c["bases"]) + 3 * (c["flags"] & 1) + 3 * (c["flags"] >> 1)
        starts = list(range(c["left_len"])) + [T - i - 31 for i in range(c["right_len"])]
        for s in ([c["left_len"] - 3] if c["flags"] & 1 else []) + ([T - c["right_len"]] if c["flags"] & 2 else []):
            offs |= {s - q for q in starts if 0 <= s - q <= 30}
    assert {0, 1, 2, 28, 29, 30} <= offs
    stage_equals_model(rfx, rows, p, 2, "residues")


def test_cut_lengths_on_word_edges_and_a_long_contig(rfx):
    rng = np.random.default_rng(13)
    p = X.default_params(40, max_iteration=1)
    rows = [end_row(rng, i, L, 40 + i, 45 - i, bool(i & 1), bool(i & 2)) for i, L in enumerate((32, 33, 62, 63, 64, 65, 3000))]
    text, out = stage_equals_model(rfx, rows, p, 2, "cut lengths")
    assert sorted(len(r[0]) + len(r[2]) for r in X.run_stages(rows, p, 2)[0]["long"]) == [32, 33, 62, 63, 64, 65, 3000]
    stage2_equals_model(rfx, text, p, 2, "cut lengths", resident=out)


def test_a_duplicated_contig_through_the_whole_chain(rfx):
    rng = np.random.default_rng(14)
    p = X.default_params(31, max_iteration=150)
    rows = genome_rows(rng, 6, 31)
    d = rand_seq(rng, 100)
    rows += [end_row(rng, 6, 0, 20, 20, contig=d, left=-1, right=-1), end_row(rng, 7, 0, 20, 20, contig=d, left=3, right=-1, fl=True)]
    text, out = stage_equals_model(rfx, rows, p, 2, "duplicate")
    c, text2 = stage2_equals_model(rfx, text, p, 2, "duplicate", resident=out)
    assert sum(ln.split(",")[1].count(d) for ln in text2.splitlines()) >= 1
    dd, _ = rfx.dedup_dev(c)
    assert 0 < dd.n <= c.n


# ---- 3. the text-buffer rule ----------------------------------------------------------------------------------------------------------
def test_the_text_buffer_rule_at_every_cap_and_alignment(rfx):
    import torch
    rng = np.random.default_rng(15)
    seqs = [rand_seq(rng, L) for L in (62, 401, 95, 1000, 64, 130, 77, 63, 99, 100, 101, 5)]
    c = rfx.contigs_pack(seqs)
    ci = c._c()
    want = np.frombuffer(X.to_text2([(s, 0, 0) for s in seqs]).encode(), np.uint8)
    n = len(want)
    for shift in range(16):
        caps = (15, 16, 17, n - 1, n) if shift % 5 else (0, 1, 15, 16, 17, n - 1, n, n + 5)
        for cap in caps:
            buf = torch.full((n + 96,), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert buf.data_ptr() % 16 == 0
            ln = C.c_int64(-77)
            st = rfx.L.rfx_dev_ext2_to_text(rfx.ctx, C.byref(ci), buf.data_ptr() + 32 + shift, cap, C.addressof(ln))
            got = buf.cpu().numpy()
            lim = min(cap, n)
            assert st == (OK if cap >= n else E_CAP) and ln.value == n, (shift, cap, st)
            assert np.array_equal(got[32 + shift:32 + shift + lim], want[:lim]), (shift, cap)
            assert (got[:32 + shift] == FILL).all() and (got[32 + shift + lim:] == FILL).all(), (shift, cap)


def host_call(rfx, fn, text, P, prm, cap, pad=16):
    off, n_rows = rfx._row_offsets(text)
    o, ln = np.full(max(cap, 0) + pad, FILL, np.uint8), C.c_int64(-77)
    st = fn(rfx.ctx, text, off.ctypes.data, n_rows, P, C.byref(prm), o.ctypes.data, cap, C.addressof(ln))
    return st, o, ln.value


def test_the_host_forms_write_nothing_into_a_short_buffer(rfx, vec):
    p, P, rows, st, ps, kmers, passes, text, rounds2, text2 = vec["k99_P2_s2_M3"]
    prm = cparams(rfx, p)
    for fn, src, want in ((rfx.L.rfx_ext_text, "".join(lines(rows)).encode(), text.encode()), (rfx.L.rfx_ext2_text, text.encode(), text2.encode())):
        n = len(want)
        for cap in (0, n - 1, n):
            st_, o, ln = host_call(rfx, fn, src, P, prm, cap)
            assert st_ == (OK if cap >= n else E_CAP) and ln == n
            assert (o == FILL).all() if cap < n else (o[:n].tobytes() == want and (o[n:] == FILL).all())


# ---- 4. contracts ----------------------------------------------------------------------------------------------------------------------
def poisoned_set(cap_n, cap_words):
    import torch
    from reflexiv_amd.api import EndextSet
    s = EndextSet(cap_n, cap_words)
    ts = s.set.tensors() + [getattr(s, a) for a in s.ARRAYS]
    for t in ts:
        t.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    return s, ts


def all_untouched(ts):
    import torch
    return all(bool((t.view(torch.uint8) == FILL).all()) for t in ts)


def small_rows():
    rng = np.random.default_rng(16)
    return [end_row(rng, 0, 70, 10, 12), end_row(rng, 1, 90, 33, 5, True, False), end_row(rng, 2, 64, 0, 40, False, True), end_row(rng, 3, 80, 7, 7, True, True),
            end_row(rng, 4, 20, 5, 5)]


def test_every_refused_argument_leaves_the_outputs_untouched(rfx):
    import torch
    L, ctx = rfx.L, rfx.ctx
    rows = small_rows()
    p = X.default_params(31, max_iteration=1)
    prm = cparams(rfx, p)
    d_text, d_off = upload(lines(rows))
    n = len(rows)
    good = dev_set(rfx, X.device_set(rows, p))
    gi = good._c()
    s, ts = poisoned_set(8, 64)
    lg, run = poisoned(8, 64), poisoned(8 * 607, 8 * 607 + 64)
    km = torch.full((8 * 606,), -1, dtype=torch.int64, device="cuda")
    buf = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nk, ln = C.c_int64(-77), C.c_int64(-77)
    from_text = lambda t, o, m, pr, so: L.rfx_dev_ext_from_text(ctx, t.data_ptr() if t is not None else None, o.data_ptr() if o is not None else None, m,   # noqa: E731
                                                                C.byref(pr) if pr is not None else None, C.byref(so) if so is not None else None)
    ends = lambda si, pr, lo=lg, k=km, cap=8 * 606, out_n=nk: L.rfx_dev_ext_contig_ends(   # noqa: E731
        ctx, C.byref(si) if si is not None else None, C.byref(pr) if pr is not None else None, C.byref(lo._c()) if lo is not None else None,
        k.data_ptr() if k is not None else None, cap, C.addressof(out_n) if out_n is not None else None)
    runf = lambda si, P, pr, ro=run: L.rfx_dev_ext_run(ctx, C.byref(si) if si is not None else None, P, C.byref(pr) if pr is not None else None,   # noqa: E731
                                                      C.byref(ro._c()) if ro is not None else None)
    assert ends(gi, prm, poisoned(8, 64), torch.empty(8 * 606, dtype=torch.int64, device="cuda")) == OK and runf(gi, 2, prm, poisoned(8 * 607, 8 * 607 + 64)) == OK
    nk.value = -77
    # parameters
    for bad in (dict(max_k=30), dict(max_k=125), dict(max_iteration=-2)):
        bp = cparams(rfx, dict(p, **bad))
        assert from_text(d_text, d_off, n, bp, s._c()) == E_ARG and ends(gi, bp) == E_ARG and runf(gi, 2, bp) == E_ARG, bad
        for fn in (L.rfx_ext_text, L.rfx_ext2_text):
            st_, o, l_ = host_call(rfx, fn, "".join(lines(rows)).encode(), 2, bp, 64)
            assert st_ == E_ARG and (o == FILL).all() and l_ == -77, bad
    for P in (0, 64, -1):
        assert runf(gi, P, prm) == E_ARG, P
        for fn in (L.rfx_ext_text, L.rfx_ext2_text):
            assert host_call(rfx, fn, "".join(lines(rows)).encode(), P, prm, 64)[0] == E_ARG, P
    # null pointers, negative counts
    assert from_text(None, d_off, n, prm, s._c()) == E_ARG and from_text(d_text, None, n, prm, s._c()) == E_ARG
    assert from_text(d_text, d_off, -1, prm, s._c()) == E_ARG and from_text(d_text, d_off, n, None, s._c()) == E_ARG and from_text(d_text, d_off, n, prm, None) == E_ARG
    no_idx = s._c()
    no_idx.new_idx = None
    assert from_text(d_text, d_off, n, prm, no_idx) == E_ARG
    assert ends(None, prm) == E_ARG and ends(gi, None) == E_ARG and ends(gi, prm, lo=None) == E_ARG and ends(gi, prm, k=None) == E_ARG
    assert ends(gi, prm, cap=-1) == E_ARG and ends(gi, prm, out_n=None) == E_ARG
    no_flags = good._c()
    no_flags.flags = None
    assert ends(no_flags, prm) == E_ARG and runf(no_flags, 2, prm) == E_ARG
    neg = good._c()
    neg.set.n = -1
    assert ends(neg, prm) == E_ARG and runf(neg, 2, prm) == E_ARG
    assert runf(None, 2, prm) == E_ARG and runf(gi, 2, None) == E_ARG and runf(gi, 2, prm, ro=None) == E_ARG
    c = good.set._c()
    assert L.rfx_dev_ext2_to_text(ctx, None, buf.data_ptr(), 256, C.addressof(ln)) == E_ARG
    assert L.rfx_dev_ext2_to_text(ctx, C.byref(c), None, 256, C.addressof(ln)) == E_ARG
    assert L.rfx_dev_ext2_to_text(ctx, C.byref(c), buf.data_ptr(), -1, C.addressof(ln)) == E_ARG
    assert L.rfx_dev_ext2_to_text(ctx, C.byref(c), buf.data_ptr(), 256, None) == E_ARG
    # a set whose word_off and len disagree, flags outside 0..3, end lengths outside 0..303 or below 3 on a flagged side, deviation 1
    for obj, field, at, value in ((good.set, "len", 1, -1), (good.set, "word_off", 0, 1), (good.set, "word_off", 2, 0), (good, "flags", 0, 4), (good, "flags", 2, -1),
                                  (good, "left_len", 0, -1), (good, "left_len", 0, 304), (good, "right_len", 0, -1), (good, "right_len", 0, 304),
                                  (good, "left_len", 1, 2), (good, "right_len", 2, 2), (good, "left_len", 0, 70 + 22 - 12 - 31), (good, "right_len", 0, 70 + 22 - 10 - 31)):
        t = getattr(obj, field)
        keep = int(t[at])
        t[at] = value
        torch.cuda.synchronize()
        assert ends(gi, prm) == E_ARG and runf(gi, 2, prm) == E_ARG, (field, at, value)
        if obj is good.set:
            assert L.rfx_dev_ext2_to_text(ctx, C.byref(c), buf.data_ptr(), 256, C.addressof(ln)) == E_ARG, (field, at, value)
        t[at] = keep
        torch.cuda.synchronize()
    good.left_len[0] = 70 + 22 - 12 - 32                           # (a cut contig of exactly 32 characters passes)
    torch.cuda.synchronize()
    assert ends(gi, prm, poisoned(8, 64), torch.empty(8 * 606, dtype=torch.int64, device="cuda")) == OK
    good.left_len[0] = 10
    torch.cuda.synchronize()
    nk.value = -77
    # rows the text path refuses
    seq = "A" * 80
    for bad in ("Contig_70_-1_2_0_5_4_0," + seq, ">Contig_70_-1_2_0_5_4," + seq, ">Contig_70_-1_2_0_5_4_0_1," + seq, ">Contig_70_-1_x_0_5_4_0," + seq,
                ">Contig_70_-1__0_5_4_0," + seq, ">Contig_70_-1_2_0_5_4_0" + seq, ">Contig_70_-1_2_0_5_4_0,(" + seq, ">Contig_70_-1_2_0_5_99999999999_0," + seq,
                ">contig_70_-1_2_0_5_4_0," + seq, ""):
        with pytest.raises(ValueError):
            X.parse_row(bad)
        t, o = upload(lines(rows + [bad]))
        assert from_text(t, o, n + 1, prm, s._c()) == E_ARG, bad
        st_, o8, l_ = host_call(rfx, L.rfx_ext_text, "".join(lines(rows + [bad])).encode(), 2, prm, 64)
        assert st_ == E_ARG and (o8 == FILL).all() and l_ == -77, bad
    st_, o8, l_ = host_call(rfx, L.rfx_ext_text, (">Contig_31_0_0_0_20_20_0," + "A" * 71 + "\n").encode(), 2, prm, 64)       # deviation 1 through the host form
    assert st_ == E_ARG and (o8 == FILL).all()
    # 2^31 rows or contigs: refused before anything is read
    assert from_text(d_text, d_off, 1 << 31, prm, s._c()) == E_LIMIT
    big = good._c()
    big.set.n = 1 << 31
    assert ends(big, prm) == E_LIMIT and runf(big, 2, prm) == E_LIMIT
    assert L.rfx_dev_ext2_to_text(ctx, C.byref(big.set), buf.data_ptr(), 256, C.addressof(ln)) == E_LIMIT
    off, _ = rfx._row_offsets("".join(lines(rows)).encode())
    o8 = np.full(64, FILL, np.uint8)
    assert L.rfx_ext_text(ctx, "".join(lines(rows)).encode(), off.ctypes.data, 1 << 31, 2, C.byref(prm), o8.ctypes.data, 64, C.addressof(ln)) == E_LIMIT
    # a contig of 2^30 bases, and one of 10,000,000 for the text of 09: word_off in step, so the layout holds and no word is read
    last = good.n - 1
    keep = int(good.set.len[last]), int(good.set.word_off[last + 1])
    for length, calls in ((1 << 30, (lambda: ends(gi, prm), lambda: runf(gi, 2, prm))), (10_000_000, ())):
        good.set.len[last] = length
        good.set.word_off[last + 1] = int(good.set.word_off[last]) + (length + 31) // 32
        torch.cuda.synchronize()
        for call in calls:
            assert call() == E_LIMIT
        assert L.rfx_dev_ext2_to_text(ctx, C.byref(c), buf.data_ptr(), 256, C.addressof(ln)) == E_LIMIT, length
    good.set.len[last], good.set.word_off[last + 1] = keep
    torch.cuda.synchronize()
    assert (o8 == FILL).all()
    assert all_untouched(ts) and untouched(lg) and untouched(run) and bool((km == -1).all()) and bool((buf == FILL).all()) and (nk.value, ln.value) == (-77, -77)


def test_the_limits_that_only_a_large_input_reaches(rfx):
    """2^32 end 31-mers, a row of 2^30 characters and 2^31 rows through the host form of 09: RFX_E_LIMIT with every output as it was.
    The sizes kernel reads no word of a contig, so 7.1 million contigs of 638 bases with ends of 303 (a cut part of 32) need their
    per-contig arrays only (about 300 MB); the row parser reads a row's ID, its first base and its last character, so the row is 1 GiB
    of one letter behind its ID."""
    import torch
    from reflexiv_amd.api import EndextSet
    L, ctx = rfx.L, rfx.ctx
    prm = cparams(rfx, X.default_params(31, max_iteration=1))
    lg, run = poisoned(8, 64), poisoned(8, 64)
    km = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    nk, ln = C.c_int64(-77), C.c_int64(-77)
    why = lambda: (L.rfx_last_error(ctx) or b"").decode()   # noqa: E731
    n = -(-(1 << 32) // 606)
    assert (n - 1) * 606 < 1 << 32 <= n * 606 and n < 1 << 31
    e = EndextSet(n, 1)
    e.set.n = n
    e.set.word_off.copy_(torch.arange(n + 1, dtype=torch.int64, device="cuda") * 20)
    e.set.len.fill_(638)
    for a in e.ARRAYS:
        getattr(e, a).fill_(303 if a in ("left_len", "right_len") else 0)
    torch.cuda.synchronize()
    ei = e._c()
    assert L.rfx_dev_ext_contig_ends(ctx, C.byref(ei), C.byref(prm), C.byref(lg._c()), km.data_ptr(), 8, C.addressof(nk)) == E_LIMIT
    assert "2^32" in why()
    assert L.rfx_dev_ext_run(ctx, C.byref(ei), 2, C.byref(prm), C.byref(run._c())) == E_LIMIT
    assert untouched(lg) and untouched(run) and bool((km == -1).all()) and nk.value == -77
    del e
    # one row of 2^30 characters behind its ID
    head = b">Contig_1_0_0_0_0_0_0,"
    text = torch.full((len(head) + (1 << 30),), ord("A"), dtype=torch.uint8, device="cuda")
    text[:len(head)] = torch.frombuffer(bytearray(head), dtype=torch.uint8).cuda()
    off = torch.tensor([0, len(head) + (1 << 30)], dtype=torch.int64, device="cuda")
    s, ts = poisoned_set(8, 64)
    so = s._c()
    so.set.n = -77
    torch.cuda.synchronize()
    assert L.rfx_dev_ext_from_text(ctx, text.data_ptr(), off.data_ptr(), 1, C.byref(prm), C.byref(so)) == E_LIMIT
    assert "2^30" in why() and int(so.set.n) == -77 and all_untouched(ts)
    del text
    # 2^31 rows through the host form of 09: refused before an offset is read
    rows = "".join(lines(small_rows())).encode()
    off8, _ = rfx._row_offsets(rows)
    o8 = np.full(64, FILL, np.uint8)
    assert L.rfx_ext2_text(ctx, rows, off8.ctypes.data, 1 << 31, 2, C.byref(prm), o8.ctypes.data, 64, C.addressof(ln)) == E_LIMIT
    assert (o8 == FILL).all() and ln.value == -77


def test_every_capacity_one_short(rfx):
    import torch
    L, ctx = rfx.L, rfx.ctx
    rows = small_rows()
    p = X.default_params(31, max_iteration=1)
    prm = cparams(rfx, p)
    d_text, d_off = upload(lines(rows))
    want = X.device_set(rows, p, False)
    m, sw = len(want), sum((len(c["bases"]) + 31) // 32 for c in want)
    assert m == len(rows) - 1
    ft = lambda so: L.rfx_dev_ext_from_text(ctx, d_text.data_ptr(), d_off.data_ptr(), len(rows), C.byref(prm), C.byref(so))   # noqa: E731
    s, ts = poisoned_set(m, sw)
    so = s._c()
    assert ft(so) == OK and (int(so.set.n), int(so.set.need_n), int(so.set.need_words)) == (m, m, sw) and not all_untouched(ts)
    for cap_n, cap_w in ((m - 1, sw), (m, sw - 1)):
        s, ts = poisoned_set(cap_n, cap_w)
        so = s._c()
        so.set.n = -77
        assert ft(so) == E_CAP and (int(so.set.need_n), int(so.set.need_words), int(so.set.n)) == (m, sw, -77) and all_untouched(ts), (cap_n, cap_w)
    good = dev_set(rfx, X.device_set(rows, p))
    gi = good._c()
    longs, kmers = X.set_contig_ends(X.device_set(rows, p), p)
    n31, lw = len(kmers), sum((len(r[2]) + 31) // 32 for r in longs)
    assert lw <= good.set.words and n31 == sum(c["left_len"] + c["right_len"] for c in want)
    for cap_k, cap_n, cap_w in ((n31, m, lw), (n31 - 1, m, lw), (n31, m - 1, lw), (n31, m, lw - 1)):
        lg = poisoned(cap_n, cap_w)
        km = torch.full((n31 + 8,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        co, nk = lg._c(), C.c_int64(-77)
        st = L.rfx_dev_ext_contig_ends(ctx, C.byref(gi), C.byref(prm), C.byref(co), km.data_ptr(), cap_k, C.addressof(nk))
        ok = (cap_k, cap_n, cap_w) == (n31, m, lw)
        assert st == (OK if ok else E_CAP) and nk.value == n31 and (int(co.n), int(co.need_words)) == (m, lw), (cap_k, cap_n, cap_w)
        assert bool((km[n31:] == -1).all()) and (ok or (untouched(lg) and bool((km == -1).all()))), (cap_k, cap_n, cap_w)
    out = rfx.ext_run(good, 2, prm)
    words = int(out.ext_off[out.n])
    for cap_n, cap_w in ((out.n, words), (out.n - 1, words), (out.n, words - 1)):
        ro = poisoned(cap_n, cap_w)
        co = ro._c()
        st = L.rfx_dev_ext_run(ctx, C.byref(gi), 2, C.byref(prm), C.byref(co))
        ok = (cap_n, cap_w) == (out.n, words)
        assert st == (OK if ok else E_CAP) and (int(co.n), int(co.need_words)) == (out.n, words) and (ok or untouched(ro)), (cap_n, cap_w)
    assert out.n <= 607 * good.n and words <= 607 * good.n + good.set.words


def test_nothing_in_is_nothing_out_through_every_entry_point(rfx):
    import torch
    p = X.default_params(31)
    prm = cparams(rfx, p)
    d_text, d_off = upload([])
    s = rfx.ext_from_text(d_text, d_off, prm)
    assert s.n == 0 and int(s.set.word_off[0]) == 0
    short = rfx.ext_from_text(*upload(lines([">Contig_1_0_0_0_30_30_0," + "A" * 61])), prm)      # every row dropped
    assert short.n == 0 and int(short.set.word_off[0]) == 0
    for e in (s, short, dev_set(rfx, [])):
        lg, d_k, nk = rfx.ext_contig_ends(e, prm)
        assert (lg.n, nk) == (0, 0)
        out = rfx.ext_run(e, 3, prm)
        assert out.n == 0 and text_of(rfx, out) == ""
        c, dl, dr = rfx.fix2_contigs(rfx.fix2_run(out, 3, prm), prm)
        assert c.n == 0 and text2_of(rfx, c) == ""
    assert rfx.ext_text(b"", 3, prm) == b"" and rfx.ext2_text(b"", 3, prm) == b""
    torch.cuda.synchronize()


# ---- 5. poisoned allocations ---------------------------------------------------------------------------------------------------------
def test_the_stages_hold_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it, so a producer that
    relied on zeroed memory for its padding bits fails the raw-word checks above.  A child process: the mask is read once per process."""
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
