"""Reads to contigs in one resident call (rfx_dev_meta_from_reduced, rfx_dev_meta_reads, rfx_meta_reads) against
the independent model (tests/meta_model.py, whose texts tests/golden/meta_vectors.npz stores and test_meta_model.py regenerates): for
every case and every stop_after the host form's text byte for byte; the device forms' set against Assembly and the report against the
model's counts; the partition rule at O = 10 against P = 10 throughout at the stage test_meta_model.py names; no reads; every refusal
with the outputs untouched; and all of it again with every allocation poisoned."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from reflexiv_amd import _lib
from tests import meta_model as MM
from tests.test_gpu_dynamic_packed import FILL, OK, E_ARG, E_CAP
from tests.test_gpu_map import dev_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "meta_vectors.npz")
CASES = ("k23_31_41_O8", "k23_31_41_O10", "k23_67_95_O10")


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


@pytest.fixture(scope="module")
def vec():
    """name -> (reads, klist, O, reduce params, params, {stage: text}, {stage: count}), from the stored vectors"""
    return MM.load_vectors(VEC)


def params_of(rfx, v, **kw):
    reads, klist, O_, rp, p = v[:5]
    return rfx.reduce_reads_params(**rp), rfx.meta_params(P=O_, min_contig=p["min_contig"], **kw)


@pytest.mark.parametrize("stage", MM.STAGES)
@pytest.mark.parametrize("case", CASES)
def test_the_host_form_writes_every_stage_of_the_model(rfx, vec, case, stage):
    v = vec[case]
    rp, mp = params_of(rfx, v, stop_after=stage)
    text, rep = rfx.meta_reads_text([r.encode() for r in v[0]], v[1], rp, mp, with_report=True)
    assert text.decode() == v[5][stage], (case, stage)
    at = MM.STAGES.index(stage)
    want = v[6]
    done = at + 1 if stage == "05FixingAgain" else at                # (05FixingAgain and 06ContigEnds are one stage's two files)
    for i, s in enumerate(MM.STAGES):
        assert rep[s] == (want[s] if i <= done else 0), (case, stage, s, rep)
    assert rep["reduced"] == want["reduced"] and rep["hits"] == (want["hits"] if at >= MM.STAGES.index("Mapping") else 0)
    assert _lib.META_STAGES == MM.STAGES


@pytest.mark.parametrize("case", CASES)
def test_the_device_forms_leave_the_assembly(rfx, vec, case):
    v = vec[case]
    reads, klist, O_ = v[:3]
    rp, mp = params_of(rfx, v)
    dw, dn, wpr = dev_reads(reads)
    longest = max(len(r) for r in reads)
    contigs, rep = rfx.meta_reads_dev(dw, dn, len(reads), wpr, longest, klist, rp, mp)
    t, n, _ = rfx.contigs_to_text_dev(contigs, v[4]["min_contig"])
    assert bytes(t[:n].cpu().numpy()).decode() == v[5]["Assembly"] != ""
    assert {s: rep[s] for s in MM.STAGES} == {s: v[6][s] for s in MM.STAGES} and rep["hits"] == v[6]["hits"] and rep["reduced"] == v[6]["reduced"]
    reduced, per_k = rfx.reduce_reads_dev(dw, dn, len(reads), wpr, longest, klist, rp)
    again, rep2 = rfx.meta_from_reduced_dev(reduced, dw, dn, len(reads), wpr, klist[-1], mp)
    assert rep2 == rep and sum(per_k) == rep["reduced"]
    for a, b in zip(again.host(), contigs.host()):
        assert np.array_equal(a, b)
    # a short d_out: the needs set, nothing written; the retry is the call again
    from reflexiv_amd.api import ContigsPacked
    import torch
    short = ContigsPacked(contigs.n - 1, contigs.words)
    for t_ in short.tensors():
        t_.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    co, ci, r = short._c(), reduced._c(), _lib.CMetaReport()
    co.n = -77
    st = rfx.L.rfx_dev_meta_from_reduced(rfx.ctx, C.byref(ci), dw.data_ptr(), dn.data_ptr(), len(reads), wpr, klist[-1], C.byref(mp), C.byref(r), C.byref(co))
    assert st == E_CAP and (int(co.need_n), int(co.need_words), int(co.n)) == (contigs.n, contigs.words, -77)
    assert all(bool((t_.view(torch.uint8) == FILL).all()) for t_ in short.tensors())


def test_the_partition_rule_shows_at_the_stage_the_model_names(rfx, vec):
    """O = 10: the rule gives (10, 8, 6, 4); P = 10 throughout gives another text from the named stage on"""
    v = vec["k23_31_41_O10"]
    stage = v[7]["rule_stage"]
    same, _ = MM.run(v[0], v[1], v[2], rule=MM.same_p, reduce_params=v[3], **v[4])
    rp, mp = params_of(rfx, v, stop_after=stage)
    got = rfx.meta_reads_text([r.encode() for r in v[0]], v[1], rp, mp).decode()
    assert got == v[5][stage] and got != same[stage]


def test_reflexiv_host_meta_and_dedup_write_the_models_files(vec, tmp_path):
    """`meta -intermediate` on the case's FASTQ writes Assembly and every file of Assembly_intermediate/; `dedup` on its 09ExtendAgain
    writes the same Assembly"""
    v = vec["k23_31_41_O10"]
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    fq, out, out2 = tmp_path / "reads.fq", tmp_path / "out", tmp_path / "out2"
    fq.write_text("".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(v[0])))
    r = subprocess.run([exe, "meta", "-fastq", str(fq), "-klist", ",".join(str(k) for k in v[1]), "-partition", str(v[2]), "-mincontig",
                        str(v[4]["min_contig"]), "-outfile", str(out), "-intermediate"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (out / "Assembly" / "part-00000").read_text() == v[5]["Assembly"] and (out / "Assembly" / "_SUCCESS").exists()
    for s in MM.STAGES[:-1]:
        d = out / "Assembly_intermediate" / s
        part = "part-00000" if s == "06ContigEnds" else "part-00000.tsv" if s == "Mapping" else "part-00000.csv"
        assert (d / part).read_text() == v[5][s] and (d / "_SUCCESS").exists(), s
    r = subprocess.run([exe, "dedup", "-kmerc", str(out / "Assembly_intermediate" / "09ExtendAgain"), "-mincontig", str(v[4]["min_contig"]), "-outfile",
                        str(out2)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (out2 / "Assembly" / "part-00000").read_text() == v[5]["Assembly"] and (out2 / "Assembly" / "_SUCCESS").exists()
    r = subprocess.run([exe, "meta"], capture_output=True, text=True)
    assert r.returncode != 0 and "-fastq" in r.stderr


def test_no_reads_give_empty_texts_and_an_empty_set(rfx):
    for stage in MM.STAGES:
        assert rfx.meta_reads_text([], (23, 31, 41), None, rfx.meta_params(stop_after=stage)) == b""
    contigs, rep = rfx.meta_reads_dev(None, None, 0, 1, 0, (23, 31, 41))
    assert contigs.n == 0 and not any(rep.values())


def test_every_refusal_leaves_the_outputs_untouched(rfx, vec):
    import torch
    from reflexiv_amd.api import ContigsPacked
    L, ctx = rfx.L, rfx.ctx
    v = vec["k23_31_41_O8"]
    reads = v[0][:40]
    dw, dn, wpr = dev_reads(reads)
    longest = max(len(r) for r in reads)
    out = ContigsPacked(64, 1024)
    for t in out.tensors():
        t.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    co = out._c()
    co.n = -77
    ks = (C.c_int * 3)(23, 31, 41)
    rp, rep = rfx.reduce_reads_params(), _lib.CMetaReport()
    dev = lambda mp, k=ks, nk=3, r=rp, w=dw.data_ptr(), o=co, rr=rep: L.rfx_dev_meta_reads(     # noqa: E731
        ctx, w, dn.data_ptr(), len(reads), wpr, longest, k, nk, C.byref(r) if r is not None else None, C.byref(mp) if mp is not None else None,
        C.byref(rr) if rr is not None else None, C.byref(o) if o is not None else None)
    P = rfx.meta_params
    for bad in (P(P=0), P(P=64), P(max_iteration=-2), P(min_contig=-1), P(map_seed=10), P(map_min_overlap=201), P(map_max_mismatch=32), P(stop_after=-1),
                P(stop_after=17), P(stop_after="09ExtendAgain"), None):
        assert dev(bad) == E_ARG, bad and [getattr(bad, f) for f, _ in bad._fields_]
    good = P()
    assert dev(good, o=None) == E_ARG and dev(good, rr=None) == E_ARG and dev(good, r=None) == E_ARG and dev(good, w=None) == E_ARG
    assert dev(good, k=(C.c_int * 3)(23, 31, 125)) == E_ARG and dev(good, k=(C.c_int * 3)(23, 25, 29)) == E_ARG and dev(good, nk=1) == E_ARG
    assert dev(good, r=rfx.reduce_reads_params(P=0)) == E_ARG
    no_len = out._c()
    no_len.len = None
    assert dev(good, o=no_len) == E_ARG
    # the host form
    bases = np.frombuffer("".join(reads).encode(), np.uint8)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    o8, ln = np.full(256, FILL, np.uint8), C.c_int64(-77)
    host = lambda mp, b=bases.ctypes.data, cap=256, l=C.addressof(ln): L.rfx_meta_reads(      # noqa: E731
        ctx, b, off.ctypes.data, len(reads), ks, 3, C.byref(rp), C.byref(mp) if mp is not None else None, None, o8.ctypes.data, cap, l)
    assert host(None) == E_ARG and host(P(stop_after=17)) == E_ARG and host(P(P=64)) == E_ARG and host(good, b=None) == E_ARG
    assert host(good, cap=-1) == E_ARG and host(good, l=None) == E_ARG
    assert ln.value == -77 and (o8 == FILL).all()
    # a short text buffer: the length set, nothing written
    text = rfx.meta_reads_text([r.encode() for r in v[0]], v[1], rfx.reduce_reads_params(**v[3]), rfx.meta_params(P=v[2], min_contig=100))
    all_reads = [r.encode() for r in v[0]]
    bases = np.frombuffer(b"".join(all_reads), np.uint8)
    off = np.zeros(len(all_reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in all_reads])
    st = L.rfx_meta_reads(ctx, bases.ctypes.data, off.ctypes.data, len(all_reads), ks, 3, C.byref(rfx.reduce_reads_params(**v[3])),
                          C.byref(rfx.meta_params(P=v[2], min_contig=100)), None, o8.ctypes.data, 256, C.addressof(ln))
    assert st == E_CAP and ln.value == len(text) > 256 and (o8 == FILL).all()
    assert all(bool((t.view(torch.uint8) == FILL).all()) for t in out.tensors()) and int(co.n) == -77


def test_the_call_holds_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it.  A child process: the
    mask is read once per process."""
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
