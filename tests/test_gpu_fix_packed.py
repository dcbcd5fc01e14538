"""rfx_dev_fix_run_packed: the contig fixing stage straight from the packed set of the last iteration, against
rfx_dev_fix_run on the rows rfx_dev_dyn_to_text writes of that set -- record for record, raw word for raw word -- and against the
string model: every case of tests/golden/fixing_vectors.npz; sets of 257 and of 4,097 records whose first and last record the length
filter drops, with keys of 22, 30, 66 and 124 bases, a left of 30001 that is clamped and a marker of ten digits; the same set with
junk in every bit behind a key's and an extension's last base; the refusals and the RFX_E_CAP rule with every output untouched; the
empty set; and all of it again with every allocation poisoned."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fixing_model as F
from tests.test_gpu_dynamic_packed import poisoned, untouched, OK, E_ARG, E_CAP, E_LIMIT
from tests.test_gpu_fixing import MARK, VEC, case_names, cparams, equals, host, lines, rand_seq, text_of
from tests.test_gpu_ksort import upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("key", "key_len", "ext", "ext_off", "ext_len", "marker", "left", "right")


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


@pytest.fixture(scope="module")
def vec():
    z = np.load(VEC)
    return {n: F.load_case(z, n) for n in case_names()}


def through_text(rfx, pk, P, cp):
    """rfx_dev_dyn_to_text -> the row offsets from the newlines, on the device -> rfx_dev_fix_run -> (the set, the text's rows)"""
    import torch
    d_text, ln = rfx.dyn_to_text_dev(pk)
    ends = torch.nonzero(d_text[:ln] == 10).flatten() + 1
    d_off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), ends.to(torch.int64)])
    torch.cuda.synchronize()
    assert int(d_off.numel()) == pk.n + 1
    return rfx.fix_run(d_text[:ln], d_off, P, cp), bytes(d_text[:ln].cpu().numpy()).decode().splitlines()


def same_sets(a, b, tag):
    assert a.n == b.n, (tag, a.n, b.n)
    for name, x, y in zip(NAMES, a.host(), b.host()):
        assert x.shape == y.shape and np.array_equal(x, y), (tag, name)


def both_ways(rfx, pk, p, P, tag):
    """-> (the packed seam's set, the rows the text seam went through)"""
    cp = cparams(rfx, p)
    want, rows = through_text(rfx, pk, P, cp)
    got = rfx.fix_run_packed(pk, P, cp)
    assert rfx.last_call_ms > 0
    same_sets(got, want, tag)
    assert got.n <= pk.n * (2 * (p["max_k"] - 30) + 1) and got.words <= got.n + pk.words + 4 * pk.n, (tag, "the capacities the header states")
    return got, rows


@pytest.mark.parametrize("case", case_names())
def test_every_case_of_the_reference_vectors(rfx, vec, case):
    p, P, rows, st, ps, kmers, passes, text = vec[case]
    pk = rfx.dyn_binarize_dev(*upload(lines(rows)), 1)              # every row, the short ones too: what an iteration leaves
    got, _ = both_ways(rfx, pk, p, P, case)
    equals(rfx, got, passes[-1], (case, "model"))
    assert text_of(rfx, got) == text


def big_set(rfx, n, mk, seed):
    """n records cut from one genome so that neighbours overlap: keys of 22, 30, 66 and 124 bases, both markers; the first and the
    last record one base short of 2 max_k; record 1 with a left of 30001, record 2 with a right of -30001, record 3 with a marker of ten
    digits (all three written into the set in HBM: the host form clamps) -> (the set, its model records as the text seam reads them)"""
    import torch
    rng = np.random.default_rng(seed)
    g = rand_seq(rng, 45 * n + 4 * mk + 400)
    recs, pos = [], 0
    for i in range(n):
        L = 2 * mk - 1 if i in (0, n - 1) else 2 * mk + 64 + int(rng.integers(0, 70))
        c = g[pos:pos + L]
        pos += int(rng.integers(15, 45))
        m = 1 + i % 2
        kl = min((22, 30, 66, 124)[i % 4], L - 1)
        key, ext = (c[:kl], c[kl:]) if m == 1 else (c[L - kl:], c[:L - kl])
        recs.append((key, m, ext, int(rng.choice(MARK)), int(rng.choice(MARK))))
    pk = rfx.dyn_pack(host(recs))
    pk.left[1], pk.right[2], pk.marker[3] = 30001, -30001, 1234567890
    torch.cuda.synchronize()
    recs[1] = recs[1][:3] + (30000, recs[1][4])
    recs[2] = recs[2][:4] + (-30000,)
    recs[3] = (recs[3][0], 123456789) + recs[3][2:]
    return pk, recs


@pytest.mark.parametrize("n", (257, 4097))
def test_sets_past_one_block_with_the_filter_the_clamp_and_every_key_length(rfx, n):
    p = F.default_params(31, scramble=2 + n % 2, max_iteration=1)
    pk, recs = big_set(rfx, n, 31, n)
    got, rows = both_ways(rfx, pk, p, 3, n)
    # the text seam read what the model reads: the clamp and the nine digits are in the ROWS only as 30001 / 1234567890
    assert ",1|30001|" in rows[1] or ",2|30001|" in rows[1]
    assert rows[3].split(",")[1].startswith("1234567890|") and len(rows) == n
    kept = [r for r in recs if len(r[0]) + len(r[2]) >= 62]
    assert len(kept) == n - 2 and {len(r[0]) for r in kept} == {22, 30, 66, 124}
    longs, kmers = F.contig_ends(kept, p)
    lg, d_k, nk = rfx.fix_contig_ends(rfx.dyn_pack(host(kept)), cparams(rfx, p))
    assert lg.n == len(longs) == n - 2 and nk == len(kmers)
    assert 0 < got.n < n + nk
    if n == 257:
        want = F.run_stages([f"{r[0]},{r[1]}|{r[3]}|{r[4]},{r[2]}" for r in recs], p, 3, order="sorted")[3][-1]
        equals(rfx, got, want, (n, "model"))


def test_junk_behind_the_last_base_of_keys_and_extensions_reaches_nothing(rfx):
    """the rows print bases only, so the text seam never sees a bit behind them; the packed seam keeps the bases and nothing else"""
    import torch
    p = F.default_params(31, max_iteration=0)
    pk, _ = big_set(rfx, 257, 31, 9)
    clean = rfx.fix_run_packed(pk, 2, cparams(rfx, p))
    key, key_len, ext, ext_off, ext_len = (x.copy() for x in pk.host()[:5])
    rng = np.random.default_rng(3)
    for i in range(pk.n):
        for j in range(4):
            left = int(key_len[i]) - 32 * j
            mask = np.uint64(0xFFFFFFFFFFFFFFFF) if left <= 0 else np.uint64(0) if left >= 32 else np.uint64((1 << (64 - 2 * left)) - 1)
            key[i, j] |= np.uint64(rng.integers(0, 1 << 63)) & mask
        tail = int(ext_len[i]) % 32
        if tail:
            ext[int(ext_off[i + 1]) - 1] |= np.uint64(rng.integers(0, 1 << 63)) & np.uint64((1 << (64 - 2 * tail)) - 1)
    pk.key[:4 * pk.n] = torch.from_numpy(key.reshape(-1).view(np.int64)).cuda()
    pk.ext[:len(ext)] = torch.from_numpy(ext.view(np.int64)).cuda()
    torch.cuda.synchronize()
    got, _ = both_ways(rfx, pk, p, 2, "junk")
    same_sets(got, clean, "junk against clean")


def test_every_refusal_and_the_capacity_rule_leave_the_outputs_untouched(rfx, vec):
    import torch
    L, ctx = rfx.L, rfx.ctx
    p, P, rows, st, ps, kmers, passes, text = vec["k41_P7_s2_M3"]
    cp = cparams(rfx, p)
    pk = rfx.dyn_binarize_dev(*upload(lines(rows)), 1)
    ci = pk._c()
    call = lambda ci_, P_, cp_, co: L.rfx_dev_fix_run_packed(ctx, ci_, P_, cp_, co)      # noqa: E731
    d = poisoned(20000, 20000)
    co = d._c()
    co.n = co.need_words = -77
    # null pointers, P, the parameters
    assert call(None, P, C.byref(cp), C.byref(co)) == E_ARG and call(C.byref(ci), P, None, C.byref(co)) == E_ARG
    assert call(C.byref(ci), P, C.byref(cp), None) == E_ARG and L.rfx_dev_fix_run_packed(None, C.byref(ci), P, C.byref(cp), C.byref(co)) == E_ARG
    for f in ("key", "ext_off", "right"):
        no = pk._c()
        setattr(no, f, None)
        assert call(C.byref(no), P, C.byref(cp), C.byref(co)) == E_ARG, f
        no = d._c()
        setattr(no, f, None)
        assert call(C.byref(ci), P, C.byref(cp), C.byref(no)) == E_ARG, f
    neg = pk._c()
    neg.n = -1
    assert call(C.byref(neg), P, C.byref(cp), C.byref(co)) == E_ARG
    for bad_p in (0, 64, -1):
        assert call(C.byref(ci), bad_p, C.byref(cp), C.byref(co)) == E_ARG, bad_p
    for mk in (30, 125, 0, -5):
        assert call(C.byref(ci), P, C.byref(rfx.fix_params(mk)), C.byref(co)) == E_ARG, mk
    assert call(C.byref(ci), P, C.byref(rfx.fix_params(41, max_iteration=-2)), C.byref(co)) == E_ARG
    # a record without an extension has no form-1 row, kept or dropped; a key of more than 124 bases; offsets that do not follow the lengths
    for t, at, value, status in ((pk.ext_len, 2, 0, E_ARG), (pk.ext_len, pk.n - 1, -4, E_ARG), (pk.key_len, 0, 125, E_LIMIT), (pk.key_len, 5, 255, E_LIMIT),
                                 (pk.ext_off, 3, int(pk.ext_off[3]) + 1, E_ARG), (pk.ext_off, 0, -1, E_ARG), (pk.ext_len, 4, int(pk.ext_len[4]) + 64, E_ARG)):
        keep = int(t[at])
        t[at] = value
        torch.cuda.synchronize()
        assert call(C.byref(ci), P, C.byref(cp), C.byref(co)) == status, (at, value)
        t[at] = keep
        torch.cuda.synchronize()
    assert untouched(d) and (int(co.n), int(co.need_words)) == (-77, -77)
    # RFX_E_CAP: n and need_words set, nothing written; with exactly the needs the call succeeds
    assert call(C.byref(ci), P, C.byref(cp), C.byref(co)) == OK
    need_n, need_w = int(co.n), int(co.need_words)
    assert 0 < need_n <= pk.n * (2 * (p["max_k"] - 30) + 1) and 0 < need_w <= need_n + pk.words + 4 * pk.n
    exact = poisoned(need_n, need_w)
    assert call(C.byref(ci), P, C.byref(cp), C.byref(exact._c())) == OK and not untouched(exact)
    for cap_n, cap_w in ((need_n - 1, need_w), (need_n, need_w - 1)):
        d = poisoned(cap_n, cap_w)
        co = d._c()
        co.n = co.need_words = -77
        assert call(C.byref(ci), P, C.byref(cp), C.byref(co)) == E_CAP, (cap_n, cap_w)
        assert (int(co.n), int(co.need_words)) == (need_n, need_w) and untouched(d), (cap_n, cap_w)


def test_an_empty_set_and_a_set_the_filter_empties(rfx):
    cp = rfx.fix_params(41)
    none = rfx.dyn_binarize_dev(*upload([]), 1)
    short = rfx.dyn_binarize_dev(*upload(["ACGTACGT,1|2|3,ACGT\n", "ACGTAC,2|-1|0,A\n"]), 1)
    for pk in (none, short):
        out = rfx.fix_run_packed(pk, 5, cp)
        assert out.n == 0 and int(out.ext_off[0]) == 0


def test_the_seam_holds_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it, so a producer that relied
    on zeroed memory for its padding bits or unused key words fails the raw-word checks above.  A child process: the mask is read once
    per process."""
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
