"""rfx_dev_endext_consensus_hits: the consensus of both ends of every contig straight from the hits of the end
mapping and the 2-bit read store, against rfx_dev_endext_consensus on the rows rfx_dev_map_to_text writes for the same contigs, reads
and hits -- word for word, offsets, lengths and flags -- and against the string models: the planted genome; a contig with no hit and
contigs with 1, 4, 5 and 9 hits (the pile-up's workgroup has 4 waves); overhangs of 1, 2, 63, 64, 65, 299, 300 and 301 bases on reads of
up to 340 bases (11 words a read), which put the read offset at 31, 0 and 1 mod 32; a read with N; junk behind every read's length; a
whole-contig target fed on both sides; 300 contigs; the refusals, a corrupted hit among them, and the capacities with every output
untouched; and all of it again with every allocation poisoned."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import endext_model as E
from tests import map_model as M
from tests.test_gpu_dynamic_packed import FILL, OK, E_ARG, E_CAP
from tests.test_gpu_endext import all_untouched, dev_contigs, poisoned_outputs
from tests.test_gpu_map import both, dev_reads, make_contigs, over_left, over_right

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


def cons_host(cons, n):
    return [x for s in (cons.left, cons.right) for x in s.host()] + [cons.flags[:n].cpu().numpy()]


def same(rfx, contigs, reads, tag, junk=None, wpr=None):
    """both ways on one input -> (the model's hits, the model's consensus per contig)"""
    c, dl, dr = dev_contigs(rfx, contigs)
    dw, dn, wpr = dev_reads(reads, wpr, junk)
    hits = rfx.map_ends(c, dl, dr, dw, dn, len(reads), wpr)
    hs = M.hits(contigs, reads)
    assert hits.n == len(hs), tag
    t, ln, off = rfx.map_to_text(c, dl, dr, dw, dn, wpr, hits)
    want = rfx.endext_consensus(c, dl, dr, t, off)
    got = rfx.endext_consensus_hits(c, dl, dr, dw, dn, wpr, hits)
    assert rfx.last_call_ms > 0
    assert got.left.n == got.right.n == c.n
    names = ("left words", "left word_off", "left len", "right words", "right word_off", "right len", "flags")
    for name, a, b in zip(names, cons_host(got, c.n), cons_host(want, c.n)):
        assert np.array_equal(a, b), (tag, name)
    assert not cons_host(got, c.n)[6].any(), (tag, "flags stay 0")
    model = E.device_consensus(contigs, [M.row_of(h) for h in hs])
    assert rfx.contigs_unpack(got.left) == [m[0] for m in model] and rfx.contigs_unpack(got.right) == [m[1] for m in model], (tag, "model")
    return hs, model


def test_the_planted_genome(rfx):
    genome, spans, contigs, reads = M.planted_case()
    hs, model = same(rfx, contigs, reads, "planted")
    assert len(hs) > 100 and all(m[0] and m[1] for m in model)
    assert {h[2] for h in hs} == {0, 1} and {h[1] & 1 for h in hs} == {0, 1}


def crafted():
    """contig 0: no hit; 1: one hit; 2: four; 3: five; 4: nine (a whole-contig target, fed on both sides); 5 (450 bases): every overhang
    of the list at its -L and at its -R; 6: a read with N at each end"""
    rng = np.random.default_rng(12)
    contigs = make_contigs(rng, [90, 100, 110, 120, 130, 450, 140])
    b = [x[1] for x in contigs]
    reads = [over_left(rng, b[1], 80, 17)]
    reads += [over_left(rng, b[2], 90, 10 + i) for i in range(4)]
    reads += [over_right(rng, b[3], 90, 20 + i) for i in range(5)]
    reads += [over_left(rng, b[4], 100, 30 + i) for i in range(5)] + [over_right(rng, b[4], 100, 25 + i) for i in range(4)]
    for over in (1, 2, 63, 64, 65, 299, 300, 301):
        n = max(100, over + 39)
        reads += [over_left(rng, b[5], n, over), over_right(rng, b[5], n, over)]
    reads += [over_left(rng, b[5], 340, 33), over_right(rng, b[5], 340, 95)]      # (past the far end of a 200-base target: a clip there)
    # N in the overhang and in the overlap, outside the seed (read bases 24..44 at the left end, 18..38 at the right end)
    for r, spots in ((over_left(rng, b[6], 70, 24), (3, 50, 66)), (over_right(rng, b[6], 70, 31), (3, 10, 50))):
        for at in spots:
            r = r[:at] + "N" + r[at + 1:]
        reads.append(r)
    return contigs, reads


def test_hit_counts_overhangs_offsets_n_and_both_sides(rfx):
    contigs, reads = crafted()
    fw = len(reads)
    reads = reads + [M.revcomp(M.norm(r)) for r in reads[::2]]       # every other read on the other strand as well
    hs, model = same(rfx, contigs, reads, "crafted", wpr=11)
    per = [sum(1 for h in hs if h[1] >> 1 == i) for i in range(len(contigs))]
    assert per[0] == 0 and model[0][:2] == ("", "") and fw < len(reads)
    assert {1, 4, 5, 9} <= {sum(1 for h in hs if h[1] >> 1 == i and h[0] < fw) for i in range(len(contigs))}, per
    assert {1, 2, 63, 64, 65, 299, 300, 301} <= {h[6] for h in hs if h[1] >> 1 == 5}
    assert {31, 0, 1} <= {h[3] % 32 for h in hs if h[1] == 10} and {h[2] for h in hs} == {0, 1}
    assert any(h[5] > 0 for h in hs) and max(len(h[8]) for h in hs) == 340
    assert model[4][0] and model[4][1], "a whole-contig target fed on both sides"
    assert per[6] >= 2 and len(model[6][0]) == 24 and len(model[6][1]) == 31 and any("N" in reads[h[0]] for h in hs), "a read with N"
    assert len(model[5][0]) == 300 == len(model[5][1]), "an overhang of 301 is cut at 300"
    # junk behind every read's length, in its last word and in the words behind it: the same result
    assert same(rfx, contigs, reads, "crafted, junk", junk=np.random.default_rng(5), wpr=12) == (hs, model)


def test_300_contigs(rfx):
    rng = np.random.default_rng(13)
    contigs = make_contigs(rng, [int(x) for x in rng.choice((70, 95, 130, 410), 300)])
    reads = []
    for i in range(0, 300, 3):
        reads += [over_left(rng, contigs[i][1], 100, 20 + i % 40), over_right(rng, contigs[299 - i][1], 120, 30 + i % 50)]
    hs, model = same(rfx, contigs, both(reads), "300 contigs")
    assert len(hs) >= 400 and sum(1 for m in model if m[0] or m[1]) >= 150 and ("", "", 0) in model


def small(rfx):
    rng = np.random.default_rng(14)
    contigs = make_contigs(rng, [70, 410])
    reads = [over_left(rng, contigs[0][1], 45, 12), M.revcomp(over_right(rng, contigs[1][1], 50, 15)), M.rand_seq(rng, 40),
             over_left(rng, contigs[1][1], 33, 2)]
    c, dl, dr = dev_contigs(rfx, contigs)
    dw, dn, wpr = dev_reads(reads)
    hits = rfx.map_ends(c, dl, dr, dw, dn, len(reads), wpr)
    assert hits.n == 3
    return c, dl, dr, dw, dn, wpr, hits


def test_every_refusal_leaves_the_outputs_untouched(rfx):
    import torch
    L, ctx = rfx.L, rfx.ctx
    c, dl, dr, dw, dn, wpr, hits = small(rfx)
    ci, hi = c._c(), hits._c()
    cons, _, ts = poisoned_outputs(16, 160, 160, 8)
    co = cons._c()
    co.left.n = co.right.n = -77
    call = lambda ci_, l, r, w, n_, wp, h, o: L.rfx_dev_endext_consensus_hits(ctx, ci_, l, r, w, n_, wp, h, o)      # noqa: E731
    A = (C.byref(ci), dl.data_ptr(), dr.data_ptr(), dw.data_ptr(), dn.data_ptr(), wpr, C.byref(hi), C.byref(co))
    for i in (0, 1, 2, 3, 4, 6, 7):
        a = list(A)
        a[i] = None
        assert call(*a) == E_ARG, i
    assert call(*A[:5], 0, *A[6:]) == E_ARG
    for field, value in (("seed", 10), ("seed", 32), ("n", -1), ("n", hits.cap_n + 1), ("read", None), ("v", None)):
        b = hits._c()
        setattr(b, field, value)
        assert call(*A[:6], C.byref(b), A[7]) == E_ARG, (field, value)
    no_flags = cons._c()
    no_flags.flags = None
    assert call(*A[:7], C.byref(no_flags)) == E_ARG
    # a hit that map_ends cannot have written, as rfx_dev_map_to_text refuses it
    for a, at, value in (("end", 0, -1), ("end", 0, 4), ("strand", 1, 2), ("strand", 1, -1), ("v", 0, 32), ("v", 2, 0), ("offset", 0, 0), ("offset", 0, 40),
                         ("offset", 1, -1), ("read", 0, -1), ("end", 2, 3)):
        t = getattr(hits, a)
        keep = int(t[at])
        t[at] = value
        torch.cuda.synchronize()
        assert call(*A) == E_ARG, (a, at, value)
        assert "rfx_dev_map_ends does not write" in L.rfx_last_error(ctx).decode()
        t[at] = keep
        torch.cuda.synchronize()
    # a read longer than its words; a contig whose word_off and len disagree under a hit
    keep = int(dn[0])
    dn[0] = 32 * wpr + 1
    torch.cuda.synchronize()
    assert call(*A) == E_ARG
    dn[0] = keep
    keep = int(c.len[0])
    c.len[0] = keep + 40
    torch.cuda.synchronize()
    assert call(*A) == E_ARG
    c.len[0] = keep
    torch.cuda.synchronize()
    # hits and no contigs
    empty = rfx.contigs_pack([])._c()
    assert call(C.byref(empty), *A[1:]) == E_ARG
    assert all_untouched(ts) and (int(co.left.n), int(co.right.n)) == (-77, -77)
    assert call(*A) == OK and not all_untouched(ts)


def test_every_capacity_one_short_and_the_empty_inputs(rfx):
    L, ctx = rfx.L, rfx.ctx
    c, dl, dr, dw, dn, wpr, hits = small(rfx)
    ci, hi = c._c(), hits._c()
    call = lambda co, cc=ci, hh=hi: L.rfx_dev_endext_consensus_hits(ctx, C.byref(cc), dl.data_ptr(), dr.data_ptr(), dw.data_ptr(), dn.data_ptr(), wpr,   # noqa: E731
                                                                     C.byref(hh), C.byref(co))
    cons, _, ts = poisoned_outputs(16, 160, 160, 8)
    co = cons._c()
    assert call(co) == OK
    n, lw, rw = int(co.left.need_n), int(co.left.need_words), int(co.right.need_words)
    assert n == c.n == int(co.left.n) == int(co.right.n) and 0 < lw <= 10 * n and 0 < rw <= 10 * n
    cons, _, ts = poisoned_outputs(n, lw, rw, 8)
    assert call(cons._c()) == OK and not all_untouched(ts)
    for cap_n, a, b in ((n - 1, lw, rw), (n, lw - 1, rw), (n, lw, rw - 1)):
        cons, _, ts = poisoned_outputs(cap_n, a, b, 8)
        co = cons._c()
        co.left.n = co.right.n = -77
        assert call(co) == E_CAP and (int(co.left.need_n), int(co.left.need_words), int(co.right.need_words), int(co.left.n)) == (n, lw, rw, -77)
        assert all_untouched(ts), (cap_n, a, b)
    # no hits: every consensus empty; no contigs and no hits: empty sets
    none = hits._c()
    none.n = 0
    cons, _, ts = poisoned_outputs(4, 8, 8, 8)
    co = cons._c()
    assert call(co, ci, none) == OK and (int(co.left.n), int(co.left.need_words), int(co.right.need_words)) == (c.n, 0, 0)
    assert cons.left.len[:c.n].cpu().tolist() == [0] * c.n == cons.right.len[:c.n].cpu().tolist() and cons.flags[:c.n].cpu().tolist() == [0] * c.n
    co = cons._c()
    assert call(co, rfx.contigs_pack([])._c(), none) == OK and (int(co.left.n), int(co.right.n)) == (0, 0)


def test_the_seam_holds_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it.  A child process: the
    mask is read once per process."""
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
