"""The end extension of contigs from alignment rows (Assembly_intermediate/07EndExtend) on packed sets in HBM (rfx_dev_endext_*,
rfx_endext_text): every entry point against its stage of the rows the reference's own classes made
(tests/golden/endext_vectors.npz) -- sets unpacked and as raw words --; the resident hand-over from rfx_dev_fix2_contigs; the host
form and reflexiv_host endextend (four columns and full SAM lines) against the stored text; the smallest shapes that can go wrong
against the string model (tests/endext_model.py, which test_endext_model.py pins to the same vectors); the text-buffer rule at any
alignment of the destination; the argument, capacity and limit contracts; and all of it again with every allocation poisoned."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import endext_model as E
from tests import fixing2_model as F2
from tests.test_gpu_dynamic_packed import words_of, FILL, OK, E_ARG, E_CAP, E_LIMIT
from tests.test_gpu_fixing import lines, rand_seq
from tests.test_gpu_ksort import upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "endext_vectors.npz")
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


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
    """every case, loaded once: name -> (max_k, contig text, row lines, consensus rows, spliced strings, text)"""
    z = np.load(VEC)
    return {n: E.load_case(z, n) for n in case_names()}


def dev_contigs(rfx, contigs):
    """[(ID, bases)] -> what rfx_dev_fix2_contigs returns: (ContigsPacked, left, right)"""
    import torch
    c = rfx.contigs_pack([b for _, b in contigs])
    lr = np.array([[int(x) for x in i.split("_")[2:4]] for i, _ in contigs], np.int32).reshape(-1, 2)
    left, right = (torch.from_numpy(np.ascontiguousarray(lr[:, j]) if len(lr) else np.zeros(1, np.int32)).cuda() for j in (0, 1))
    torch.cuda.synchronize()
    return c, left, right


def rows_up(row_lines):
    return upload([r + "\n" for r in row_lines])


def packed_equals(rfx, c, seqs, tag):
    """a packed contig set in HBM is the list of sequences: through rfx_dev_contigs_unpack, and word for word the numpy packer's (so
    every padding bit is 0), with the offsets and the lengths"""
    assert c.n == len(seqs), (tag, c.n, len(seqs))
    assert rfx.contigs_unpack(c) == list(seqs), tag
    words, woff, ln = c.host()
    want = [words_of(np.array([CODE[ch] for ch in s], np.uint64)) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(w) for w in want])
    assert np.array_equal(woff, off) and np.array_equal(ln, np.array([len(s) for s in seqs], np.int64)), tag
    assert np.array_equal(words, np.concatenate(want) if want else np.zeros(0, np.uint64)), (tag, "words")


def stage_equals_model(rfx, contigs, row_lines, max_k, tag):
    """the three device entry points and the host form on one input against the string model -> the text"""
    c, dl, dr = dev_contigs(rfx, contigs)
    want = E.device_consensus(contigs, row_lines)
    cons = rfx.endext_consensus(c, dl, dr, *rows_up(row_lines))
    packed_equals(rfx, cons.left, [w[0] for w in want], (tag, "left consensus"))
    packed_equals(rfx, cons.right, [w[1] for w in want], (tag, "right consensus"))
    assert cons.flags[:c.n].cpu().tolist() == [w[2] for w in want], (tag, "flags")
    assert cons.left.words <= 10 * c.n and cons.right.words <= 10 * c.n
    recs = E.device_set(contigs, row_lines, max_k)
    s = rfx.endext_contigs(c, dl, dr, cons, max_k)
    packed_equals(rfx, s.set, [r["bases"] for r in recs], (tag, "spliced"))
    assert s.set.words <= c.words + 20 * c.n
    got = s.host()
    for a in s.ARRAYS:
        assert got[a].tolist() == [r[a] for r in recs], (tag, a)
    t, n = rfx.endext_to_text(s)
    text = bytes(t[:n].cpu().numpy()).decode()
    assert text == E.set_text(recs), (tag, "text")
    ctext = "".join(f"{i},{b}\n" for i, b in contigs)
    assert text == E.run_text(ctext, row_lines, max_k), (tag, "the string model's text")
    assert rfx.endext_text(ctext.encode(), "".join(r + "\n" for r in row_lines).encode(), max_k).decode() == text, (tag, "host form")
    return text


# ---- 1. every entry point against the reference's classes ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", case_names())
def test_every_entry_point_equals_its_stage_of_the_reference(rfx, vec, case):
    mk, ctext, row_lines, cons, spliced, text = vec[case]
    contigs = E.contigs_of_text(ctext)
    assert stage_equals_model(rfx, contigs, row_lines, mk, case) == text
    assert rfx.last_call_ms > 0
    # the stored consensus rows and spliced strings, not only the model's: the literals in front of a flagged consensus
    by = {}
    for ident, s in cons:
        by.setdefault(ident, {})[s[0]] = s[2:]
    c, dl, dr = dev_contigs(rfx, contigs)
    out = rfx.endext_consensus(c, dl, dr, *rows_up(row_lines))
    lc, rc, fl = rfx.contigs_unpack(out.left), rfx.contigs_unpack(out.right), out.flags[:c.n].cpu().tolist()
    for i, (ident, _) in enumerate(contigs):
        want = by.get(ident, {"L": "", "R": ""})
        assert ("l1-" * (fl[i] & 1) + lc[i], "r1-" * (fl[i] >> 1) + rc[i]) == (want["L"], want["R"]), (case, ident)
    s = rfx.endext_contigs(c, dl, dr, out, mk)
    kept = [x for x in spliced if len(x.split(",")[1]) >= 2 * mk]
    assert [x.split(",")[1].replace("-1l", "").replace("r1-", "") for x in kept] == rfx.contigs_unpack(s.set), case


def test_fix2_contigs_feed_the_stage_with_no_text_in_between(rfx, vec):
    """rows of 04Fixing -> rfx_dev_fix2_* -> the contigs in HBM -> rfx_dev_endext_* equals 05FixingAgain's text -> rfx_endext_text"""
    z2 = np.load(os.path.join(ROOT, "tests", "golden", "fixing2_vectors.npz"))
    for case in ("fix_new_k31_P2_s2_M-1", "fix_fix_k41_P7_s2_M3"):
        mk, ctext, row_lines, cons, spliced, text = vec[case]
        p, P, rows = F2.load_case(z2, case[4:])[:3]
        prm = rfx.fix_params(p["max_k"], scramble=p["scramble"], max_iteration=p["max_iteration"])
        c, dl, dr = rfx.fix2_contigs(rfx.fix2_run(rfx.fix2_binarize(*upload(lines(rows))), P, prm), prm)
        out = rfx.endext_consensus(c, dl, dr, *rows_up(row_lines))
        t, n = rfx.endext_to_text(rfx.endext_contigs(c, dl, dr, out, mk))
        assert bytes(t[:n].cpu().numpy()).decode() == text == rfx.endext_text(ctext.encode(), "".join(r + "\n" for r in row_lines).encode(), mk).decode()


def sam_lines(row_lines):
    out = ["@HD\tVN:1.6\tSO:unsorted", "@SQ\tSN:x\tLN:1"]
    for i, (name, start, cigar, seq) in enumerate(E.split_rows(row_lines)):
        out.append(f"read{i}\t{16 * (i % 2)}\t{name}\t{start}\t60\t{cigar}\t*\t0\t0\t{seq}\t*\tNM:i:0")
        if i % 7 == 0:
            out.append(f"unmapped{i}\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII")
    return out


@pytest.mark.parametrize("full_sam", (False, True))
@pytest.mark.parametrize("case", ("crafted_k50", "fix_new_k99_P63_s2_M3"))
def test_reflexiv_host_endextend_writes_the_stored_text(vec, tmp_path, case, full_sam):
    import subprocess
    mk, ctext, row_lines, cons, spliced, text = vec[case]
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    d = tmp_path / "05FixingAgain"
    d.mkdir()
    (d / "part-00000.csv").write_text(ctext)
    sam, out = tmp_path / "rows.tsv", tmp_path / "out"
    sam.write_text("".join(r + "\n" for r in (sam_lines(row_lines) if full_sam else row_lines)))
    if full_sam:
        assert E.sam_to_rows(sam_lines(row_lines)) == ["\t".join(r) for r in E.split_rows(row_lines)]
    r = subprocess.run([exe, "endextend", "-kmerc", str(d), "-sam", str(sam), "-klist", f"23,{mk}", "-outfile", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = out / "Assembly_intermediate" / "07EndExtend"
    assert (d / "part-00000.csv").read_text() == text and (d / "_SUCCESS").exists()


# ---- 2. the smallest shapes that can go wrong, against the string model ---------------------------------------------------------------
def make_contigs(rng, lengths, lr=None):
    out = []
    for i, L in enumerate(lengths):
        l, r = lr[i % len(lr)] if lr else (int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
        out.append((f"Contig_{L}_{l}_{r}_{i}", rand_seq(rng, L)))
    return out


def left_row(rng, contig, cnt, seq=None):
    """a row that adds cnt >= 2 bases to the left table of a contig"""
    ident, bases = contig
    name = ident + ("-L" if len(bases) >= 400 else "")
    return f"{name}\t1\t{cnt}S30M\t{seq or rand_seq(rng, cnt + 30)}"


def right_row(rng, contig, cnt, seq=None):
    """a row that adds cnt >= 1 bases to the right table"""
    ident, bases = contig
    two = len(bases) >= 400
    ref = 200 if two else len(bases)
    return f"{ident + ('-R' if two else '')}\t{ref - 30 + 1}\t30M{cnt}S\t{seq or rand_seq(rng, cnt + 30)}"


@pytest.mark.parametrize("n", (0, 1, 2, 255, 256, 257))
def test_contig_counts_around_a_block(rfx, n):
    rng = np.random.default_rng(100 + n)
    contigs = make_contigs(rng, [int(x) for x in rng.integers(62, 140, n)])
    rows = []
    for c in contigs:
        for _ in range(int(rng.integers(0, 3))):
            rows.append(left_row(rng, c, int(rng.integers(2, 60))))
            rows.append(right_row(rng, c, int(rng.integers(1, 60))))
    rows += ["Contig_62_0_0_999\t1\t5S30M\t" + "A" * 35]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    text = stage_equals_model(rfx, contigs, rows, 31, n)
    assert text.count("\n") == n
    if n >= 11:                                                      # the order is the strings': ..._10 ahead of ..._2, L = 100 ahead of 99
        ids = [t.split(",")[0] for t in text.splitlines()]
        assert [int(i.split("_")[4]) for i in ids] != sorted(int(i.split("_")[4]) for i in ids)
        assert [int(i.split("_")[7]) for i in ids] == list(range(n))


def test_row_counts_that_wrap_the_workgroups_row_loop(rfx):
    """0, 1, 63, 64, 65 and 5,000 rows on one contig each (a wave takes every fourth row), unsorted, with markers among them"""
    rng = np.random.default_rng(3)
    counts = (0, 1, 63, 64, 65, 5000, 3, 4, 5)
    contigs = make_contigs(rng, [450 if i % 2 else 90 for i in range(len(counts))])
    rows = []
    for c, k in zip(contigs, counts):
        truth_l, truth_r = rand_seq(rng, 80), rand_seq(rng, 80)
        for j in range(k):
            cnt = int(rng.integers(2, 70))
            noisy = lambda s: "".join(ch if rng.random() > 0.2 else "ACGTn"[int(rng.integers(0, 5))] for ch in s)      # noqa: E731
            rows.append(left_row(rng, c, cnt, noisy(truth_l[:cnt][::-1]) + rand_seq(rng, 30)) if j % 2 else
                        right_row(rng, c, cnt, rand_seq(rng, 30) + noisy(truth_r[:cnt])))
            if j % 50 == 7:
                rows.append(f"{c[0]}{'-L' if len(c[1]) >= 400 else ''}\t0\t*\tL")
    rows = [rows[i] for i in rng.permutation(len(rows))]
    stage_equals_model(rfx, contigs, rows, 31, "row counts")


def test_consensus_lengths_and_every_residue_of_the_left_seam(rfx):
    """consensus lengths 0, 1 (right), 2 (left), 31..33, 299 and 300, the left length at every residue mod 32 (the splice's seams are
    funnel shifts), contig lengths at 30..34 and 62..66 mod 32 -- flagged and not"""
    rng = np.random.default_rng(4)
    lefts = [0] + list(range(2, 35)) + [63, 64, 65, 299, 300, 301, 310]
    rights = [0, 1, 2, 31, 32, 33, 299, 300, 301]
    lens = [62, 63, 64, 65, 66, 94, 95, 96, 97, 98, 130, 400, 401, 431, 432, 433]
    contigs = make_contigs(rng, [lens[i % len(lens)] for i in range(len(lefts))], lr=[(-1, -1), (0, 0), (1, 1), (2, 2), (-30000, 30000)])
    rows = []
    for i, c in enumerate(contigs):
        if lefts[i]:
            rows.append(left_row(rng, c, lefts[i]))
        r = rights[i % len(rights)]
        if r:
            rows.append(right_row(rng, c, r))
        side = "-L" if len(c[1]) >= 400 else ""
        if i % 3 == 0:
            rows += [f"{c[0]}{side}\t0\t*\tL"] * 2
        if i % 4 == 0:
            rows += [f"{c[0]}{'-R' if side else ''}\t0\t*\tR"] * (2 + i % 2)
    text = stage_equals_model(rfx, contigs, rows, 31, "lengths")
    assert "-1l" in text and "r1-" in text
    want = E.device_consensus(contigs, rows)
    assert {len(w[0]) % 32 for w in want} == set(range(32)) and {299, 300} <= {len(w[0]) for w in want} and {1, 299, 300} <= {len(w[1]) for w in want}


def test_the_length_filter_counts_text_characters(rfx):
    """2 max_k - 1, 2 max_k: bases alone, with a consensus, and with the three literal characters of a flagged side"""
    rng = np.random.default_rng(6)
    mk = 40
    contigs = make_contigs(rng, [79, 80, 77, 76, 74, 73, 60, 1, 0, 1])
    rows = [left_row(rng, contigs[2], 3), left_row(rng, contigs[3], 3)]
    # an original of one base or none is no row of the output, whatever its consensus, and takes no index (:433, :513): the three
    # sort ahead of every other ID, so counting them would move every index below by three
    rows += [left_row(rng, contigs[7], 90), right_row(rng, contigs[7], 90), right_row(rng, contigs[8], 120)]
    rows += [f"{contigs[4][0]}\t0\t*\tL-R"] * 2 + [f"{contigs[5][0]}\t0\t*\tL-R"] * 2
    text = stage_equals_model(rfx, contigs, rows, mk, "filter")
    assert [int(t.split("_")[4]) for t in text.splitlines()] == [4, 2, 1]          # 74 + 6, 77 + 3, 80: in the order of the strings
    assert [int(t.split(",")[0].split("_")[7]) for t in text.splitlines()] == [2, 4, 6]     # the index runs over the dropped ones too


# ---- 3. the text-buffer rule ----------------------------------------------------------------------------------------------------------
def test_the_text_buffer_rule_at_every_cap_and_alignment(rfx):
    import torch
    rng = np.random.default_rng(5)
    contigs = make_contigs(rng, [62, 401, 95, 400, 130, 77, 1000, 64])
    rows = [left_row(rng, contigs[1], 40), right_row(rng, contigs[1], 17), right_row(rng, contigs[4], 300), f"{contigs[2][0]}\t0\t*\tL-R",
            f"{contigs[2][0]}\t0\t*\tL-R", left_row(rng, contigs[2], 9)]
    c, dl, dr = dev_contigs(rfx, contigs)
    s = rfx.endext_contigs(c, dl, dr, rfx.endext_consensus(c, dl, dr, *rows_up(rows)), 31)
    si = s._c()
    want = np.frombuffer(E.set_text(E.device_set(contigs, rows, 31)).encode(), np.uint8)
    n = len(want)
    for shift in range(16):
        caps = (n, n - 1) if shift % 5 else (0, 1, 15, 16, 17, 33, n - 17, n - 1, n, n + 5)
        for cap in caps:
            buf = torch.full((n + 96,), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert buf.data_ptr() % 16 == 0
            ln = C.c_int64(-77)
            st = rfx.L.rfx_dev_endext_to_text(rfx.ctx, C.byref(si), buf.data_ptr() + 32 + shift, cap, C.addressof(ln))
            got = buf.cpu().numpy()
            lim = min(cap, n)
            assert st == (OK if cap >= n else E_CAP) and ln.value == n, (shift, cap, st)
            assert np.array_equal(got[32 + shift:32 + shift + lim], want[:lim]), (shift, cap)
            assert (got[:32 + shift] == FILL).all() and (got[32 + shift + lim:] == FILL).all(), (shift, cap)
    # the host form with a short buffer writes nothing
    ct, rt = "".join(f"{i},{b}\n" for i, b in contigs).encode(), "".join(r + "\n" for r in rows).encode()
    (oc, nc), (orr, nr) = rfx._row_offsets(ct), rfx._row_offsets(rt)
    for cap in (0, n - 1, n):
        o, ln = np.full(n + 16, FILL, np.uint8), C.c_int64(0)
        st = rfx.L.rfx_endext_text(rfx.ctx, ct, oc.ctypes.data, nc, rt, orr.ctypes.data, nr, 31, o.ctypes.data, cap, C.addressof(ln))
        assert st == (OK if cap >= n else E_CAP) and ln.value == n
        assert (o == FILL).all() if cap < n else (np.array_equal(o[:n], want) and (o[n:] == FILL).all())


# ---- 4. contracts ----------------------------------------------------------------------------------------------------------------------
def poisoned_outputs(cap_n, lw, rw, sw):
    import torch
    from reflexiv_amd.api import EndextConsensus, EndextSet
    cons, s = EndextConsensus(cap_n, lw, rw), EndextSet(cap_n, sw)
    ts = cons.left.tensors() + cons.right.tensors() + [cons.flags] + s.set.tensors() + [getattr(s, a) for a in s.ARRAYS]
    for t in ts:
        t.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    return cons, s, ts


def all_untouched(ts):
    import torch
    return all(bool((t.view(torch.uint8) == FILL).all()) for t in ts)


def small_input(rfx):
    rng = np.random.default_rng(8)
    contigs = make_contigs(rng, [62, 401, 95, 400, 130, 77])
    rows = [left_row(rng, contigs[1], 40), right_row(rng, contigs[1], 17), right_row(rng, contigs[4], 33), left_row(rng, contigs[0], 5)]
    return contigs, rows


def test_every_refused_argument_leaves_the_outputs_untouched(rfx):
    import torch
    L, ctx = rfx.L, rfx.ctx
    contigs, rows = small_input(rfx)
    c, dl, dr = dev_contigs(rfx, contigs)
    ci = c._c()
    d_text, d_off = rows_up(rows)
    good = rfx.endext_consensus(c, dl, dr, d_text, d_off)
    gset = rfx.endext_contigs(c, dl, dr, good, 31)
    cons, s, ts = poisoned_outputs(16, 160, 160, 400)
    buf = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ln = C.c_int64(-77)
    con = lambda t, o, n: L.rfx_dev_endext_consensus(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), t.data_ptr(), o.data_ptr(), n, C.byref(cons._c()))   # noqa: E731
    # the stated deviations: rows that are no markers and that the reference would throw on
    name = contigs[0][0]
    bad_rows = [f"{name}\t1\t10S50\t{'A' * 60}", f"{name}\t1\tS50M\t{'A' * 60}", f"{name}\t1\t10s50M\t{'A' * 60}", f"{name}\t1\t\t{'A' * 60}",
                f"{name}\t1\t10S 50M\t{'A' * 60}", f"{name}\t1\t1000000000S5M\t{'A' * 60}", f"{name}\tx\t10S50M\t{'A' * 60}", f"{name}\t\t10S50M\t{'A' * 60}",
                f"{name}\t1.0\t10S50M\t{'A' * 60}", f"{name}\t99999999999\t10S50M\t{'A' * 60}", f"{name}\t1\t10S50M\t{'A' * 9}",
                f"{name}\t33\t30M10S\t{'A' * 9}", f"{name}\t1\t10S50M\tL-R-"]
    for bad in bad_rows:
        t, o = rows_up(rows + [bad])
        assert con(t, o, len(rows) + 1) == E_ARG, bad
        ct, rt = "".join(f"{i},{b}\n" for i, b in contigs).encode(), "".join(r + "\n" for r in rows + [bad]).encode()
        (oc, nc), (orr, nr) = rfx._row_offsets(ct), rfx._row_offsets(rt)
        o8 = np.full(64, FILL, np.uint8)
        assert L.rfx_endext_text(ctx, ct, oc.ctypes.data, nc, rt, orr.ctypes.data, nr, 31, o8.ctypes.data, 64, C.addressof(ln)) == E_ARG and (o8 == FILL).all(), bad
    # the same rows are no error as markers' neighbours: a marker, an ignored name, a row of three fields
    for fine in (f"{name}\tx\t10S50\tL", f"Contig_62_9_9_0\t1\t10S50\t{'A' * 60}", f"Contig_1_2_3_4\tx\t??\tA", f"{name}\t1\t10S50"):
        t, o = rows_up(rows + [fine])
        ok = rfx.endext_consensus(c, dl, dr, t, o)
        assert rfx.contigs_unpack(ok.left) == rfx.contigs_unpack(good.left) and rfx.contigs_unpack(ok.right) == rfx.contigs_unpack(good.right), fine
    # the host form's contig rows
    rt = "".join(r + "\n" for r in rows).encode()
    orr, nr = rfx._row_offsets(rt)
    for bad in ("Contig_5_0_0_0,ACGT\n", "Contig_4_0_0_1,ACGT\n", "Contig_4_00_0_0,ACGT\n", "Contig_4_0_0_0;ACGT\n", "Contig_4_0_0,ACGT\n", "ACGT\n",
                "Contig_4_0_0_0,ACGN\n", "Contig_4_0_0_0,acgt\n", "Contig_40_0_0_0," + "ACGT" * 9 + "AC-T\n"):
        ct = bad.encode()
        oc, nc = rfx._row_offsets(ct)
        o8 = np.full(64, FILL, np.uint8)
        assert L.rfx_endext_text(ctx, ct, oc.ctypes.data, nc, rt, orr.ctypes.data, nr, 31, o8.ctypes.data, 64, C.addressof(ln)) == E_ARG and (o8 == FILL).all(), bad
    # max_k, null pointers, negative counts
    gi, si = good._c(), s._c()
    ct, rt = "".join(f"{i},{b}\n" for i, b in contigs).encode(), "".join(r + "\n" for r in rows).encode()
    (oc, nc), (orr, nr) = rfx._row_offsets(ct), rfx._row_offsets(rt)
    o8 = np.full(64, FILL, np.uint8)
    for mk in (30, 125):
        assert L.rfx_dev_endext_contigs(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), C.byref(gi), mk, C.byref(si)) == E_ARG
        assert L.rfx_endext_text(ctx, ct, oc.ctypes.data, nc, rt, orr.ctypes.data, nr, mk, o8.ctypes.data, 64, C.addressof(ln)) == E_ARG, mk
    n = len(rows)
    assert L.rfx_dev_endext_consensus(ctx, None, dl.data_ptr(), dr.data_ptr(), d_text.data_ptr(), d_off.data_ptr(), n, C.byref(cons._c())) == E_ARG
    assert L.rfx_dev_endext_consensus(ctx, C.byref(ci), None, dr.data_ptr(), d_text.data_ptr(), d_off.data_ptr(), n, C.byref(cons._c())) == E_ARG
    assert L.rfx_dev_endext_consensus(ctx, C.byref(ci), dl.data_ptr(), None, d_text.data_ptr(), d_off.data_ptr(), n, C.byref(cons._c())) == E_ARG
    assert L.rfx_dev_endext_consensus(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), None, d_off.data_ptr(), n, C.byref(cons._c())) == E_ARG
    assert L.rfx_dev_endext_consensus(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), d_text.data_ptr(), None, n, C.byref(cons._c())) == E_ARG
    assert L.rfx_dev_endext_consensus(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), d_text.data_ptr(), d_off.data_ptr(), -1, C.byref(cons._c())) == E_ARG
    assert L.rfx_dev_endext_consensus(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), d_text.data_ptr(), d_off.data_ptr(), n, None) == E_ARG
    no_flags = cons._c()
    no_flags.flags = None
    assert L.rfx_dev_endext_consensus(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), d_text.data_ptr(), d_off.data_ptr(), n, C.byref(no_flags)) == E_ARG
    assert L.rfx_dev_endext_contigs(ctx, None, dl.data_ptr(), dr.data_ptr(), C.byref(gi), 31, C.byref(si)) == E_ARG
    assert L.rfx_dev_endext_contigs(ctx, C.byref(ci), None, dr.data_ptr(), C.byref(gi), 31, C.byref(si)) == E_ARG
    assert L.rfx_dev_endext_contigs(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), None, 31, C.byref(si)) == E_ARG
    assert L.rfx_dev_endext_contigs(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), C.byref(gi), 31, None) == E_ARG
    no_idx = s._c()
    no_idx.new_idx = None
    assert L.rfx_dev_endext_contigs(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), C.byref(gi), 31, C.byref(no_idx)) == E_ARG
    fewer = good._c()
    fewer.left.n = c.n - 1
    assert L.rfx_dev_endext_contigs(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), C.byref(fewer), 31, C.byref(si)) == E_ARG
    gs = gset._c()
    assert L.rfx_dev_endext_to_text(ctx, None, buf.data_ptr(), 256, C.addressof(ln)) == E_ARG
    assert L.rfx_dev_endext_to_text(ctx, C.byref(gs), None, 256, C.addressof(ln)) == E_ARG
    assert L.rfx_dev_endext_to_text(ctx, C.byref(gs), buf.data_ptr(), -1, C.addressof(ln)) == E_ARG
    assert L.rfx_dev_endext_to_text(ctx, C.byref(gs), buf.data_ptr(), 256, None) == E_ARG
    # sets whose word_off and len disagree, a consensus longer than 300 bases, flags that are none
    for obj, field, at, value in ((c, "len", 1, -1), (c, "word_off", 0, 1), (c, "word_off", 2, 0), (good.left, "len", 1, 301), (good.left, "len", 1, 7),
                                  (good.right, "word_off", 3, 9), (good, "flags", 0, 4)):
        t = getattr(obj, field)
        keep = int(t[at])
        t[at] = value
        torch.cuda.synchronize()
        assert L.rfx_dev_endext_contigs(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), C.byref(gi), 31, C.byref(si)) == E_ARG, (field, at, value)
        t[at] = keep
        torch.cuda.synchronize()
    for obj, field, at, value in ((gset.set, "len", 1, -1), (gset.set, "word_off", 0, 1), (gset.set, "word_off", 2, 0), (gset, "flags", 0, 4), (gset, "left_len", 1, 500),
                                  (gset, "right_len", 1, -1)):
        t = getattr(obj, field)
        keep = int(t[at])
        t[at] = value
        torch.cuda.synchronize()
        assert L.rfx_dev_endext_to_text(ctx, C.byref(gs), buf.data_ptr(), 256, C.addressof(ln)) == E_ARG, (field, at, value)
        t[at] = keep
        torch.cuda.synchronize()
    # 2^31 rows, 2^31 contigs: refused before anything is read, by every entry point
    assert con(d_text, d_off, 1 << 31) == E_LIMIT
    big = c._c()
    big.n = 1 << 31
    assert L.rfx_dev_endext_consensus(ctx, C.byref(big), dl.data_ptr(), dr.data_ptr(), d_text.data_ptr(), d_off.data_ptr(), n, C.byref(cons._c())) == E_LIMIT
    bigc = good._c()
    bigc.left.n = bigc.right.n = 1 << 31
    assert L.rfx_dev_endext_contigs(ctx, C.byref(big), dl.data_ptr(), dr.data_ptr(), C.byref(bigc), 31, C.byref(si)) == E_LIMIT
    bigs = gset._c()
    bigs.set.n = 1 << 31
    assert L.rfx_dev_endext_to_text(ctx, C.byref(bigs), buf.data_ptr(), 256, C.addressof(ln)) == E_LIMIT
    assert L.rfx_endext_text(ctx, ct, oc.ctypes.data, 1 << 31, rt, orr.ctypes.data, nr, 31, o8.ctypes.data, 64, C.addressof(ln)) == E_LIMIT
    assert L.rfx_endext_text(ctx, ct, oc.ctypes.data, nc, rt, orr.ctypes.data, 1 << 31, 31, o8.ctypes.data, 64, C.addressof(ln)) == E_LIMIT
    # a contig of 2^30 bases, its word_off in step (the layout is checked before a word is read): the splice and the text writer.
    # (The host form would need a row of 2^30 characters; its parser refuses such a row as it refuses any other malformed one.)
    for obj, call in ((c, lambda: L.rfx_dev_endext_contigs(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), C.byref(gi), 31, C.byref(si))),
                      (gset.set, lambda: L.rfx_dev_endext_to_text(ctx, C.byref(gs), buf.data_ptr(), 256, C.addressof(ln)))):
        last = obj.n - 1
        keep = int(obj.len[last]), int(obj.word_off[last + 1])
        obj.len[last] = 1 << 30
        obj.word_off[last + 1] = int(obj.word_off[last]) + (1 << 25)
        torch.cuda.synchronize()
        assert call() == E_LIMIT
        obj.len[last], obj.word_off[last + 1] = keep
        torch.cuda.synchronize()
    assert (o8 == FILL).all()
    assert all_untouched(ts) and bool((buf == FILL).all()) and ln.value == -77


def test_every_capacity_one_short(rfx):
    L, ctx = rfx.L, rfx.ctx
    contigs, rows = small_input(rfx)
    c, dl, dr = dev_contigs(rfx, contigs)
    ci = c._c()
    d_text, d_off = rows_up(rows)
    con = lambda co: L.rfx_dev_endext_consensus(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), d_text.data_ptr(), d_off.data_ptr(), len(rows), C.byref(co))   # noqa: E731
    cons, s, ts = poisoned_outputs(16, 160, 160, 400)
    co = cons._c()
    assert con(co) == OK
    n, lw, rw = int(co.left.need_n), int(co.left.need_words), int(co.right.need_words)
    assert n == c.n == int(co.left.n) == int(co.right.n) and 0 < lw <= 10 * n and 0 < rw <= 10 * n
    good = rfx.endext_consensus(c, dl, dr, d_text, d_off)
    gi = good._c()
    spl = lambda so: L.rfx_dev_endext_contigs(ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), C.byref(gi), 31, C.byref(so))   # noqa: E731
    so = s._c()
    assert spl(so) == OK
    m, sw = int(so.set.need_n), int(so.set.need_words)
    assert m == int(so.set.n) == c.n and 0 < sw <= c.words + 20 * c.n
    cons, s, ts = poisoned_outputs(n, lw, rw, sw)
    assert con(cons._c()) == OK and spl(s._c()) == OK and not all_untouched(ts)
    for cap_n, a, b in ((n - 1, lw, rw), (n, lw - 1, rw), (n, lw, rw - 1)):
        cons, s, ts = poisoned_outputs(cap_n, a, b, sw)
        co = cons._c()
        co.left.n = co.right.n = -77
        assert con(co) == E_CAP and (int(co.left.need_n), int(co.left.need_words), int(co.right.need_words), int(co.left.n)) == (n, lw, rw, -77)
        assert all_untouched(ts), (cap_n, a, b)
    for cap_n, a in ((m - 1, sw), (m, sw - 1)):
        cons, s, ts = poisoned_outputs(cap_n, lw, rw, a)
        so = s._c()
        so.set.n = -77
        assert spl(so) == E_CAP and (int(so.set.need_n), int(so.set.need_words), int(so.set.n)) == (m, sw, -77)
        assert all_untouched(ts), (cap_n, a)


# ---- 5. poisoned allocations ---------------------------------------------------------------------------------------------------------
def test_the_stage_holds_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it, so a producer that
    relied on zeroed memory for its padding bits fails the raw-word checks above.  A child process: the mask is read once per process."""
    import subprocess
    import sys
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
