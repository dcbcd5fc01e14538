"""The second contig fixing stage (Assembly_intermediate/05FixingAgain, 06ContigEnds) on packed sets in HBM (rfx_dev_fix2_*,
rfx_fix2_text): every operator against its stage of the rows the reference's own classes made
(tests/golden/fixing2_vectors.npz) -- packed sets unpacked field by field and as raw words, the contigs through
rfx_dev_contigs_unpack and as raw words, every loop round through rfx_dev_fix2_run stopped behind it; the resident hand-over from
rfx_dev_fix_run; the host form and reflexiv_host fixing2 against both stored texts; the smallest shapes that can go wrong against
the string model (tests/fixing2_model.py, which test_fixing2_model.py pins to the same vectors); the text-buffer rule at any
alignment of the destination; the argument, capacity and limit contracts; and all of it again with every allocation poisoned."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import fixing2_model as F
from tests import fixing_model as F1
from tests.test_gpu_dynamic_packed import poisoned, untouched, words_of, FILL, OK, E_ARG, E_CAP, E_LIMIT
from tests.test_gpu_fixing import equals, host, lines, rand_seq
from tests.test_gpu_ksort import upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "fixing2_vectors.npz")
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
    """every case, loaded once: name -> (params, P, rows, binarized, [(perm, part starts, records)], text, ends)"""
    z = np.load(VEC)
    return {n: F.load_case(z, n) for n in case_names()}


def cparams(rfx, p):
    return rfx.fix_params(p["max_k"], scramble=p.get("scramble", 2), max_iteration=p.get("max_iteration", 150))


def contigs_equal(rfx, c, dl, dr, cs, tag):
    """the packed contig set in HBM is the contig list: through rfx_dev_contigs_unpack, and word for word the numpy packer's (so
    every padding bit is 0), with the offsets, the lengths and left / right"""
    assert c.n == len(cs), (tag, c.n, len(cs))
    assert rfx.contigs_unpack(c) == [x[0] for x in cs], tag
    words, woff, ln = c.host()
    want = [words_of(np.array([CODE[ch] for ch in x[0]], np.uint64)) for x in cs]
    off = np.zeros(len(cs) + 1, np.int64)
    off[1:] = np.cumsum([len(w) for w in want])
    assert np.array_equal(woff, off) and np.array_equal(ln, np.array([len(x[0]) for x in cs], np.int64)), tag
    assert np.array_equal(words, np.concatenate(want) if want else np.zeros(0, np.uint64)), (tag, "words")
    assert dl[:c.n].cpu().tolist() == [x[1] for x in cs] and dr[:c.n].cpu().tolist() == [x[2] for x in cs], (tag, "left / right")


def both_texts(rfx, c, dl, dr):
    t, n = rfx.fix2_to_text(c, dl, dr)
    e, m = rfx.fix2_ends_text(c, dl, dr)
    return bytes(t[:n].cpu().numpy()).decode(), bytes(e[:m].cpu().numpy()).decode()


def stage_equals_model(rfx, recs, p, tag):
    """rfx_dev_fix2_contigs and both text writers on a packed set against the string model -> (the contigs, the texts)"""
    cs = F.contigs(recs, p)
    c, dl, dr = rfx.fix2_contigs(rfx.dyn_pack(host(recs)), cparams(rfx, p))
    contigs_equal(rfx, c, dl, dr, cs, tag)
    text, ends = both_texts(rfx, c, dl, dr)
    assert text == F.to_text(cs), (tag, "05FixingAgain")
    assert ends == F.ends_text(cs), (tag, "06ContigEnds")
    return cs, text, ends


def records(rng, lengths, markers=(1, 2), lr=None):
    """records in the form of 04Fixing (30-base keys) whose contigs have the given lengths"""
    out = []
    for i, L in enumerate(lengths):
        s, m = rand_seq(rng, L), markers[i % len(markers)]
        l, r = lr[i % len(lr)] if lr else (int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
        out.append((s[:30], 1, s[30:], l, r) if m == 1 else (s[L - 30:], 2, s[:L - 30], l, r))
    return out


# ---- 1. every operator against the reference's classes -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", case_names())
def test_every_operator_equals_its_stage_of_the_reference(rfx, vec, case):
    p, P, rows, recs, passes, text, ends = vec[case]
    b = rfx.fix2_binarize(*upload(lines(rows)))
    equals(rfx, b, recs, (case, "binarized"))
    # every round: rfx_dev_fix2_run stopped behind it
    for i in range(len(passes)):
        out = rfx.fix2_run(b, P, cparams(rfx, dict(p, max_iteration=i)))
        equals(rfx, out, passes[i][2], (case, "run to round", i))
    out = rfx.fix2_run(b, P, cparams(rfx, p))
    last = passes[-1][2] if passes else recs
    equals(rfx, out, last, (case, "run"))
    assert out.n <= b.n and out.words <= b.words
    # the contigs and both texts, from the reference's last record set and from the device's own
    cs = F.contigs(last, p)
    for src, tag in ((rfx.dyn_pack(host(last)), "packed reference"), (out, "resident")):
        c, dl, dr = rfx.fix2_contigs(src, cparams(rfx, p))
        contigs_equal(rfx, c, dl, dr, cs, (case, tag))
        assert c.words <= src.words + src.n                        # the bound the header states for 30-base keys
        assert both_texts(rfx, c, dl, dr) == (text, ends), (case, tag)


@pytest.mark.parametrize("case", case_names())
def test_the_host_form_writes_both_stored_texts(rfx, vec, case):
    p, P, rows, recs, passes, text, ends = vec[case]
    got = rfx.fix2_text("".join(lines(rows)).encode(), P, cparams(rfx, p))
    assert (got[0].decode(), got[1].decode()) == (text, ends)
    assert rfx.last_call_ms > 0


@pytest.mark.parametrize("case", ["k41_P7_s2_M3", "k31_P7_s3_M0", "k32_P2_s3_M150"])
def test_the_first_stage_hands_its_packed_set_over_without_text(rfx, vec, case):
    """rfx_dev_fix_run -> rfx_dev_fix2_run on the packed set equals rfx_dev_fix_run -> text -> rfx_dev_fix2_binarize -> rfx_dev_fix2_run,
    and both equal the stored last round of the case whose input is that text"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixing_vectors.npz"))
    p1, P1, rows1 = F1.load_case(z, case)[:3]
    p, P, rows, recs, passes, text, ends = vec["fix_" + case]
    assert (p, P) == (p1, P1)
    fixed = rfx.fix_run(*upload(lines(rows1)), P, cparams(rfx, p))
    resident = rfx.fix2_run(fixed, P, cparams(rfx, p))
    d_text, ln = rfx.dyn_to_text_dev(fixed)
    t = bytes(d_text[:ln].cpu().numpy()).decode()
    assert t.splitlines() == rows
    through_text = rfx.fix2_run(rfx.fix2_binarize(*upload(t.splitlines(True))), P, cparams(rfx, p))
    last = passes[-1][2] if passes else recs
    equals(rfx, resident, last, (case, "resident"))
    equals(rfx, through_text, last, (case, "through the text"))
    for a, b in zip(resident.host(), through_text.host()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", ["fix_k41_P7_s2_M3", "new_k99_P63_s2_M3", "new_k31_P2_s2_M-1"])
def test_reflexiv_host_fixing2_writes_both_files(vec, tmp_path, case):
    import subprocess
    p, P, rows, recs, passes, text, ends = vec[case]
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    src, out = tmp_path / "part-00000.csv", tmp_path / "out"
    src.write_text("".join(lines(rows)))
    r = subprocess.run([exe, "fixing2", "-kmerc", str(src), "-klist", f"23,{p['max_k']}", "-partition", str(P), "-maxiter", str(p["max_iteration"]),
                        "-scramble", str(p["scramble"]), "-outfile", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = out / "Assembly_intermediate"
    assert (d / "05FixingAgain" / "part-00000.csv").read_text() == text and (d / "05FixingAgain" / "_SUCCESS").exists()
    assert (d / "06ContigEnds" / "part-00000").read_text() == ends and (d / "06ContigEnds" / "_SUCCESS").exists()


def test_reflexiv_host_fixing_then_fixing2_reproduces_a_stored_case(vec, tmp_path):
    import subprocess
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixing_vectors.npz"))
    p, P, rows1 = F1.load_case(z, "k32_P1_s2_M3")[:3]
    text, ends = vec["fix_k32_P1_s2_M3"][5:]
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    src, out = tmp_path / "part-00000.csv", tmp_path / "out"
    src.write_text("".join(lines(rows1)))
    common = ["-klist", f"23,{p['max_k']}", "-partition", str(P), "-maxiter", str(p["max_iteration"]), "-scramble", str(p["scramble"]), "-outfile", str(out)]
    for cmd, inp in (("fixing", str(src)), ("fixing2", str(out / "Assembly_intermediate" / "04Fixing"))):
        r = subprocess.run([exe, cmd, "-kmerc", inp] + common, capture_output=True, text=True)
        assert r.returncode == 0, (cmd, r.stderr)
    d = out / "Assembly_intermediate"
    assert (d / "05FixingAgain" / "part-00000.csv").read_text() == text and (d / "06ContigEnds" / "part-00000").read_text() == ends


# ---- 2. the smallest shapes that can go wrong: against the model ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 3000])
def test_contig_counts_around_the_block_size(rfx, n):
    """a third of the contigs is dropped; idx runs over 9 -> 10, 99 -> 100 and 999 -> 1000 (n = 3,000), L over 99 -> 100, and left /
    right over every sign, so that the records of both texts start at every residue mod 16"""
    rng = np.random.default_rng(100 + n)
    p = F.default_params(41)
    recs = records(rng, [int(rng.integers(60, 120)) for _ in range(n)], lr=[(-1, -1), (0, 5), (-30000, 30000), (12, -7), (3, 0)])
    cs, text, ends = stage_equals_model(rfx, recs, p, ("count", n))
    assert len(cs) < n or n < 255
    if n == 3000:
        for t in (text, ends):
            starts = np.concatenate([[0], np.flatnonzero(np.frombuffer(t.encode(), np.uint8)[:-1] == 10) + 1])
            assert set(int(s) % 16 for s in starts) == set(range(16))
        assert len(cs) > 1000 and {99, 100} <= {len(c[0]) for c in cs}


def test_a_set_where_no_contig_survives(rfx):
    rng = np.random.default_rng(7)
    p = F.default_params(64)
    cs, text, ends = stage_equals_model(rfx, records(rng, [31, 60, 127, 100, 127]), p, "no survivor")
    assert cs == [] and text == "" and ends == ""
    assert rfx.fix2_text(b"", 3, cparams(rfx, p)) == (b"", b"")
    b = rfx.fix2_binarize(*upload([]))
    out = rfx.fix2_run(b, 5, cparams(rfx, p))
    c, dl, dr = rfx.fix2_contigs(out, cparams(rfx, p))
    assert (b.n, out.n, c.n) == (0, 0, 0) and int(out.ext_off[0]) == 0 and int(c.word_off[0]) == 0
    assert both_texts(rfx, c, dl, dr) == ("", "")


def test_every_residue_of_the_extension_and_the_edges_of_both_rules(rfx):
    """marker 2 with ext_len % 32 at every residue (the key then begins at every position of a word), marker 1 too; L = 399 / 400 /
    401 and 999 / 1000; the length filter at 2 max_k - 1 / 2 max_k / 2 max_k + 1"""
    rng = np.random.default_rng(11)
    p = F.default_params(31)
    lengths = [30 + e for e in range(32, 97)] + [399, 400, 401, 999, 1000, 61, 62, 63]
    for markers in ((2,), (1,), (1, 2)):
        cs, text, ends = stage_equals_model(rfx, records(rng, lengths, markers=markers), p, ("residues", markers))
        assert len(cs) == len(lengths) - 1 and ends.count("-L\n") == 4
    # contigs of one word or less, and keys of other lengths: rfx_dev_fix2_contigs takes any packed set
    p = F.default_params(31)
    recs = [(rand_seq(rng, kl), 1 + i % 2, rand_seq(rng, el), i, -i) for i, (kl, el) in
            enumerate([(124, 0), (124, 1), (97, 31), (64, 64), (33, 29), (32, 30), (31, 31), (1, 61), (96, 3), (124, 500), (65, 65)])]
    stage_equals_model(rfx, recs, p, "any key length")


@pytest.mark.parametrize("max_k", [31, 64, 124])
def test_a_3000_base_contig(rfx, max_k):
    rng = np.random.default_rng(max_k)
    p = F.default_params(max_k)
    lengths = [3000, 2 * max_k, 3017, 2 * max_k - 1, 3031, 3032, 3033, 400]
    cs, text, ends = stage_equals_model(rfx, records(rng, lengths), p, ("3000 bases", max_k))
    assert len(cs) == 7 and ends.count("-R\n") == 6
    # the same contigs through the loop: a set the loop has nothing to merge in comes out as contigs unchanged
    rows = [f"{k},{m}|{l}|{r},{e}\n" for k, m, e, l, r in records(rng, lengths)]
    got = rfx.fix2_text("".join(rows).encode(), 2, cparams(rfx, dict(p, max_iteration=3)))
    assert (got[0].decode(), got[1].decode()) == tuple(F.run_text(rows, dict(p, max_iteration=3), 2))


# ---- 3. the text-buffer rule ----------------------------------------------------------------------------------------------------------
def test_the_text_buffer_rule_at_every_cap_and_alignment(rfx):
    """cap of 0, 1, len - 1, len and values that are no multiple of 16, with d_text offset by 0..15 bytes into a poisoned buffer:
    the bytes below min(cap, len) are the text's, nothing before the buffer, at cap or past it is written"""
    import torch
    rng = np.random.default_rng(5)
    p = F.default_params(31)
    recs = records(rng, [62, 401, 95, 400, 130, 77, 1000, 64])
    cs = F.contigs(recs, p)
    c, dl, dr = rfx.fix2_contigs(rfx.dyn_pack(host(recs)), cparams(rfx, p))
    ci = c._c()
    for fn, want in ((rfx.L.rfx_dev_fix2_to_text, F.to_text(cs)), (rfx.L.rfx_dev_fix2_ends_text, F.ends_text(cs))):
        want = np.frombuffer(want.encode(), np.uint8)
        n = len(want)
        for shift in range(16):
            caps = (n, n - 1) if shift % 5 else (0, 1, 15, 16, 17, 33, n - 17, n - 1, n, n + 5)
            for cap in caps:
                buf = torch.full((n + 96,), FILL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                assert buf.data_ptr() % 16 == 0
                ln = C.c_int64(-77)
                st = fn(rfx.ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), buf.data_ptr() + 32 + shift, cap, C.addressof(ln))
                got = buf.cpu().numpy()
                lim = min(cap, n)
                assert st == (OK if cap >= n else E_CAP) and ln.value == n, (shift, cap, st)
                assert np.array_equal(got[32 + shift:32 + shift + lim], want[:lim]), (shift, cap)
                assert (got[:32 + shift] == FILL).all() and (got[32 + shift + lim:] == FILL).all(), (shift, cap)


def test_the_host_form_with_a_short_buffer_writes_neither(rfx, vec):
    p, P, rows, recs, passes, text, ends = vec["new_k31_P7_s3_M150"]
    t = "".join(lines(rows)).encode()
    off, n = rfx._row_offsets(t)
    cp = cparams(rfx, p)
    for cap1, cap2 in ((len(text) - 1, len(ends)), (len(text), len(ends) - 1), (0, 0)):
        o1, o2 = np.full(len(text) + 16, FILL, np.uint8), np.full(len(ends) + 16, FILL, np.uint8)
        l1, l2 = C.c_int64(0), C.c_int64(0)
        st = rfx.L.rfx_fix2_text(rfx.ctx, t, off.ctypes.data, n, P, C.byref(cp), o1.ctypes.data, cap1, C.addressof(l1), o2.ctypes.data, cap2, C.addressof(l2))
        assert st == E_CAP and (l1.value, l2.value) == (len(text), len(ends)) and (o1 == FILL).all() and (o2 == FILL).all()
    o1, o2 = np.full(len(text) + 16, FILL, np.uint8), np.full(len(ends) + 16, FILL, np.uint8)
    st = rfx.L.rfx_fix2_text(rfx.ctx, t, off.ctypes.data, n, P, C.byref(cp), o1.ctypes.data, len(text), C.addressof(l1), o2.ctypes.data, len(ends), C.addressof(l2))
    assert st == OK and o1[:len(text)].tobytes().decode() == text and o2[:len(ends)].tobytes().decode() == ends
    assert (o1[len(text):] == FILL).all() and (o2[len(ends):] == FILL).all()


# ---- 4. contracts ----------------------------------------------------------------------------------------------------------------------
def poisoned_contigs(cap_n, cap_words):
    import torch
    from reflexiv_amd.api import ContigsPacked
    c = ContigsPacked(cap_n, cap_words)
    l, r = torch.empty(max(1, cap_n), dtype=torch.int32, device="cuda"), torch.empty(max(1, cap_n), dtype=torch.int32, device="cuda")
    for t in c.tensors() + [l, r]:
        t.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    return c, l, r


def contigs_untouched(c, l, r):
    import torch
    return all(bool((t.view(torch.uint8) == FILL).all()) for t in c.tensors() + [l, r])


def test_every_refused_argument_leaves_the_outputs_untouched(rfx, vec):
    import torch
    p, P, rows, recs, passes, text, ends = vec["fix_k41_P7_s2_M3"]
    L, ctx = rfx.L, rfx.ctx
    cp = cparams(rfx, p)
    d_text, d_off = upload(lines(rows))
    b = rfx.fix2_binarize(d_text, d_off)
    bi = b._c()
    d = poisoned(20000, 40000)
    oc, ol, orr = poisoned_contigs(2000, 40000)
    good, gl, gr = rfx.fix2_contigs(b, cp)
    gi = good._c()
    buf = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ln = C.c_int64(-77)
    run = lambda prm, PP: L.rfx_dev_fix2_run(ctx, C.byref(bi), PP, C.byref(prm), C.byref(d._c()))               # noqa: E731
    con = lambda prm: L.rfx_dev_fix2_contigs(ctx, C.byref(bi), C.byref(prm), C.byref(oc._c()), ol.data_ptr(), orr.data_ptr())   # noqa: E731
    # the parameters
    for bad in (dict(max_iteration=-2), dict(max_k=30), dict(max_k=125)):
        assert run(cparams(rfx, dict(p, **bad)), P) == E_ARG, bad
    for bad in (dict(max_k=30), dict(max_k=125)):
        assert con(cparams(rfx, dict(p, **bad))) == E_ARG, bad
    for bad_p in (0, 64, -1):
        assert run(cp, bad_p) == E_ARG, bad_p
    o, off = np.full(64, FILL, np.uint8), np.array([0, 40], np.int64)
    row = ("A" * 30 + ",1|2|3,ACGTACGT\n").encode()
    for prm, PP in ((cp, 0), (cp, 64), (cparams(rfx, dict(p, max_iteration=-2)), 1), (cparams(rfx, dict(p, max_k=125)), 1)):
        assert L.rfx_fix2_text(ctx, row, off.ctypes.data, 1, PP, C.byref(prm), o.ctypes.data, 64, C.addressof(ln), o.ctypes.data, 64, C.addressof(ln)) == E_ARG
    # null pointers
    assert L.rfx_dev_fix2_binarize(ctx, None, d_off.data_ptr(), len(rows), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix2_binarize(ctx, d_text.data_ptr(), None, len(rows), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix2_binarize(ctx, d_text.data_ptr(), d_off.data_ptr(), len(rows), None) == E_ARG
    assert L.rfx_dev_fix2_binarize(ctx, d_text.data_ptr(), d_off.data_ptr(), -1, C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix2_run(ctx, None, P, C.byref(cp), C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix2_run(ctx, C.byref(bi), P, None, C.byref(d._c())) == E_ARG
    assert L.rfx_dev_fix2_run(ctx, C.byref(bi), P, C.byref(cp), None) == E_ARG
    no_key = d._c()
    no_key.key = None
    assert L.rfx_dev_fix2_run(ctx, C.byref(bi), P, C.byref(cp), C.byref(no_key)) == E_ARG
    assert L.rfx_dev_fix2_contigs(ctx, None, C.byref(cp), C.byref(oc._c()), ol.data_ptr(), orr.data_ptr()) == E_ARG
    assert L.rfx_dev_fix2_contigs(ctx, C.byref(bi), None, C.byref(oc._c()), ol.data_ptr(), orr.data_ptr()) == E_ARG
    assert L.rfx_dev_fix2_contigs(ctx, C.byref(bi), C.byref(cp), None, ol.data_ptr(), orr.data_ptr()) == E_ARG
    assert L.rfx_dev_fix2_contigs(ctx, C.byref(bi), C.byref(cp), C.byref(oc._c()), None, orr.data_ptr()) == E_ARG
    assert L.rfx_dev_fix2_contigs(ctx, C.byref(bi), C.byref(cp), C.byref(oc._c()), ol.data_ptr(), None) == E_ARG
    for fn in (L.rfx_dev_fix2_to_text, L.rfx_dev_fix2_ends_text):
        assert fn(ctx, None, gl.data_ptr(), gr.data_ptr(), buf.data_ptr(), 256, C.addressof(ln)) == E_ARG
        assert fn(ctx, C.byref(gi), None, gr.data_ptr(), buf.data_ptr(), 256, C.addressof(ln)) == E_ARG
        assert fn(ctx, C.byref(gi), gl.data_ptr(), None, buf.data_ptr(), 256, C.addressof(ln)) == E_ARG
        assert fn(ctx, C.byref(gi), gl.data_ptr(), gr.data_ptr(), None, 256, C.addressof(ln)) == E_ARG
        assert fn(ctx, C.byref(gi), gl.data_ptr(), gr.data_ptr(), buf.data_ptr(), -1, C.addressof(ln)) == E_ARG
        assert fn(ctx, C.byref(gi), gl.data_ptr(), gr.data_ptr(), buf.data_ptr(), 256, None) == E_ARG
        # a contig set whose word_off and len disagree
        for field, at, value in (("len", 1, -1), ("len", 0, 64 * 1000), ("word_off", 0, 1), ("word_off", 2, 0)):
            t = getattr(good, field)
            keep = int(t[at])
            t[at] = value
            torch.cuda.synchronize()
            assert fn(ctx, C.byref(gi), gl.data_ptr(), gr.data_ptr(), buf.data_ptr(), 256, C.addressof(ln)) == E_ARG, (field, at)
            t[at] = keep
            torch.cuda.synchronize()
    # the stated deviation: a key that is not 30 bases long, a row without an extension; a sub-k-mer of more than 124 bases
    rng = np.random.default_rng(2)
    for key, ext, want in ((29, 80, E_ARG), (31, 80, E_ARG), (30, 0, E_ARG), (125, 80, E_LIMIT)):
        bad_rows = lines(rows[:3]) + [f"{rand_seq(rng, key)},1|2|3,{rand_seq(rng, ext)}\n"]
        t, o4 = upload(bad_rows)
        assert L.rfx_dev_fix2_binarize(ctx, t.data_ptr(), o4.data_ptr(), 4, C.byref(d._c())) == want, (key, ext)
        raw = "".join(bad_rows).encode()
        ho, hn = rfx._row_offsets(raw)
        assert L.rfx_fix2_text(ctx, raw, ho.ctypes.data, hn, P, C.byref(cp), o.ctypes.data, 64, C.addressof(ln), o.ctypes.data, 64, C.addressof(ln)) == want
    for recs2 in ([("A" * 30, 1, "ACGT", 1, 1), ("C" * 31, 1, "ACGT", 1, 1)], [("A" * 30, 1, "", 1, 1)]):
        ci = rfx.dyn_pack(host(recs2))._c()
        assert L.rfx_dev_fix2_run(ctx, C.byref(ci), 1, C.byref(cp), C.byref(d._c())) == E_ARG
    assert untouched(d) and contigs_untouched(oc, ol, orr) and bool((buf == FILL).all()) and ln.value == -77 and (o == FILL).all()


def test_every_capacity_one_short(rfx, vec):
    """cap_n = need - 1, then cap_words = need - 1: RFX_E_CAP with the needs set and every output tensor (0xA5) as it was; with exactly
    the needs the same call succeeds"""
    p, P, rows, recs, passes, text, ends = vec["fix_k41_P7_s2_M3"]
    L, ctx = rfx.L, rfx.ctx
    cp = cparams(rfx, p)
    d_text, d_off = upload(lines(rows))
    b = rfx.fix2_binarize(d_text, d_off)
    bi = b._c()
    calls = {"binarize": lambda co: L.rfx_dev_fix2_binarize(ctx, d_text.data_ptr(), d_off.data_ptr(), len(rows), C.byref(co)),
             "run": lambda co: L.rfx_dev_fix2_run(ctx, C.byref(bi), P, C.byref(cp), C.byref(co))}
    bound = {"binarize": (len(rows), len(rows) + int(d_text.numel()) // 32), "run": (b.n, b.words)}
    for name, call in calls.items():
        co = poisoned(20000, 40000)._c()
        assert call(co) == OK, name
        need_n, need_w = int(co.n), int(co.need_words)
        assert 0 < need_n <= bound[name][0] and 0 < need_w <= bound[name][1], (name, need_n, need_w)
        exact = poisoned(need_n, need_w)
        assert call(exact._c()) == OK and not untouched(exact), name
        for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
            d = poisoned(cap_n, cap_w)
            co = d._c()
            co.n = co.need_words = -77
            assert call(co) == E_CAP and (int(co.n), int(co.need_words)) == (need_n, need_w) and untouched(d), (name, cap_n, cap_w)
    run = rfx.fix2_run(b, P, cp)
    ri = run._c()
    con = lambda co, l, r: L.rfx_dev_fix2_contigs(ctx, C.byref(ri), C.byref(cp), C.byref(co), l.data_ptr(), r.data_ptr())      # noqa: E731
    c, l, r = poisoned_contigs(2000, 40000)
    co = c._c()
    assert con(co, l, r) == OK
    need_n, need_w = int(co.need_n), int(co.need_words)
    assert 0 < need_n == int(co.n) <= run.n and 0 < need_w <= run.words + run.n
    c, l, r = poisoned_contigs(need_n, need_w)
    assert con(c._c(), l, r) == OK and not contigs_untouched(c, l, r)
    for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
        c, l, r = poisoned_contigs(cap_n, cap_w)
        co = c._c()
        co.n = co.need_n = co.need_words = -77
        assert con(co, l, r) == E_CAP and (int(co.need_n), int(co.need_words), int(co.n)) == (need_n, need_w, -77)
        assert contigs_untouched(c, l, r), (cap_n, cap_w)


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
    assert " passed" in r.stdout and "failed" not in r.stdout
