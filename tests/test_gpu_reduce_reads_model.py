"""Reduce from reads in one resident call (rfx_dev_reduce_reads / rfx_reduce_reads) against an INDEPENDENT model of the
whole call: tests/reduce_reads_model.py composes the CPU oracle's counters and the string models of the mercy, sorting and reduction stages
(each pinned to vectors the reference's own classes made) from the reads to the text of every Count_<k>_reduced, and
tests/golden/reduce_reads_vectors.npz holds its texts.  Nothing of the library makes the expected result, except that the texts are put
into the record form by rfx_dev_dyn_binarize form 0 (pinned in tests/test_gpu_dynamic_packed.py) for the set comparison.

The read sets are chosen for what tests/test_gpu_reduce_reads.py's own reads cannot show (tests/test_reduce_reads_model.py asserts it of
each on the CPU): `forked` lets the E of a LATER k reach the output, so a driver that ignored the rule behind the first k fails here;
`doubled` overflows the counter's first capacity at every k, so rr_sorted's second count runs; `edges` has reads at both counters' skip
rules; `sensitive` has mercy rows."""
import os
import subprocess
import sys

import pytest

from tests import reduce_reads_model as RR
from tests.test_gpu_ksort import upload
from tests.test_gpu_ksort_counts import same_set
from tests.test_gpu_map import dev_reads

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = RR.cases()


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


@pytest.fixture(scope="module")
def vectors():
    return RR.load_vectors(os.path.join(HERE, "golden", "reduce_reads_vectors.npz"))


def first_difference(got, want):
    for i, (a, b) in enumerate(zip(got.splitlines(), want.splitlines())):
        if a != b:
            return i, a, b
    return min(got.count("\n"), want.count("\n")), "(rows: %d)" % got.count("\n"), "(rows: %d)" % want.count("\n")


@pytest.mark.parametrize("name", list(CASES))
def test_the_device_equals_the_model(rfx, vectors, name):
    """the text form byte for byte, and the device form as the set that form 0 makes of the model's texts, array by array"""
    rset, klist, kw = CASES[name]
    reads, want = vectors[0][rset], vectors[1][name]
    prm = rfx.reduce_reads_params(**kw)
    got = [t.decode() for t in rfx.reduce_reads_text([r.encode() for r in reads], klist, prm)]
    for k, g, w in zip(klist, got, want):
        assert g == w, (name, f"Count_{k}_reduced", first_difference(g, w))
    if reads:
        dw, dn, wpr = dev_reads(reads)
        dev, per_k = rfx.reduce_reads_dev(dw, dn, len(reads), wpr, max(len(r) for r in reads), klist, prm)
    else:
        dev, per_k = rfx.reduce_reads_dev(None, None, 0, 1, 0, klist, prm)
    assert per_k == [t.count("\n") for t in want], name
    rows = [r for t in want for r in t.splitlines(keepends=True)]
    same_set(dev, rfx.dyn_binarize_dev(*upload(rows), 0), name)
    assert dev.n == len(rows)


def test_reflexiv_host_reduce_from_a_fastq_on_a_list_that_reaches_61(tmp_path, vectors):
    """`reflexiv_host reduce -fastq F -klist 23,67,95 -partition 8`: every Count_<k>_reduced/part-00000.csv is the model's text.  (The
    klist mode of the command applies no E rule, so it cannot stand in for the expected files on such a list.)"""
    exe = os.path.join(os.path.dirname(HERE), "reflexiv_amd", "reflexiv_host")
    reads, want = vectors[0]["forked"], vectors[1]["forked_k23_67_95_P8"]
    fq = tmp_path / "forked.fq"
    fq.write_text("".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)))
    out = tmp_path / "out"
    r = subprocess.run([exe, "reduce", "-fastq", str(fq), "-klist", "23,67,95", "-partition", "8", "-outfile", str(out)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for k, w in zip((23, 67, 95), want):
        got = (out / f"Count_{k}_reduced" / "part-00000.csv").read_text()
        assert got == w, (k, first_difference(got, w))
        assert (out / f"Count_{k}_reduced" / "_SUCCESS").exists()


def test_everything_again_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is 0xA5 before the library uses it.  A child process: the mask is read
    once per process"""
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k", "not poisoned"],
                       env=env, cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
