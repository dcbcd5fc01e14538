"""The Python wrappers that grow their output and call again (reflexiv_amd/api.py, Reflexiv._grow_call): each of
the nine kinds of wrapper once with its default output and once with an `out=` of capacity 1 in contigs / records / hits and 1 in
words -- and a one-element d_kmers where the wrapper takes one --, so the C call answers RFX_E_CAP and the wrapper has to build a
larger output from the needs the call reported.  Both calls return the same contents, the second returns a new object, and
last_call_ms is set.  The other test files drive RFX_E_CAP through the C ABI; nothing else drives this path.  The inputs are the
smallest that need more than 1 of each kind: four contigs of 62..130 bases at max_k = 31 and a dozen reads."""
import numpy as np
import pytest

from tests import map_model as M
from tests.test_gpu_endext import dev_contigs
from tests.test_gpu_extend import genome_rows
from tests.test_gpu_fixing import contig_rows, host, lines
from tests.test_gpu_fixing2 import records
from tests.test_gpu_ksort import upload
from tests.test_gpu_map import dev_reads, make_contigs, over_left, over_right

pytestmark = pytest.mark.gpu

MAX_K = 31
LENGTHS = [62, 77, 100, 130]


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


@pytest.fixture(scope="module")
def prm(rfx):
    return rfx.fix_params(MAX_K, max_iteration=2)


@pytest.fixture(scope="module")
def mapped(rfx):
    """four contigs as rfx_dev_fix2_contigs returns them, a dozen reads that hang over their ends, and the rows of the end mapping"""
    rng = np.random.default_rng(27)
    contigs = make_contigs(rng, LENGTHS)
    reads = []
    for _, b in contigs:
        reads += [over_left(rng, b, 50, 15), over_right(rng, b, 55, 20), M.revcomp(over_left(rng, b, 60, 25))]
    c, dl, dr = dev_contigs(rfx, contigs)
    dw, dn, wpr = dev_reads(reads)
    hits = rfx.map_ends(c, dl, dr, dw, dn, len(reads), wpr)
    t, _, off = rfx.map_to_text(c, dl, dr, dw, dn, wpr, hits)
    return c, dl, dr, (dw, dn, len(reads), wpr), (t, off)


def content(x):
    """everything in use of an output object: [(name, int or numpy array)] -- n, the first n entries of every array, the word_off[n] words"""
    from reflexiv_amd.api import ContigsPacked, DynPacked, EndextConsensus, EndextSet, MapHits
    if isinstance(x, (DynPacked, ContigsPacked)):
        return [("n", x.n)] + list(zip(x.FIELDS, x.host()))
    if isinstance(x, EndextConsensus):
        return [("left." + k, v) for k, v in content(x.left)] + [("right." + k, v) for k, v in content(x.right)] + [("flags", x.flags[:x.left.n].cpu().numpy())]
    if isinstance(x, EndextSet):
        return content(x.set) + sorted(x.host().items())
    assert isinstance(x, MapHits), type(x)
    return [("n", x.n), ("seed", x.seed)] + sorted(x.host().items())


def same(a, b, tag):
    ca, cb = content(a), content(b)
    assert [k for k, _ in ca] == [k for k, _ in cb], tag
    for (k, va), (_, vb) in zip(ca, cb):
        assert np.array_equal(va, vb), (tag, k, np.asarray(va).tolist()[:12], np.asarray(vb).tolist()[:12])


def grows(rfx, tag, call, short, more_than_one):
    """call(None) and call(short): the same contents out of a new object, last_call_ms set; more_than_one(result): the sizes that
    make `short` short"""
    want = call(None)
    assert all(v > 1 for v in more_than_one(want)), (tag, more_than_one(want))
    rfx.last_call_ms = None
    got = call(short)
    assert rfx.last_call_ms is not None and rfx.last_call_ms > 0, tag
    assert got is not short, tag
    same(want, got, tag)
    return want, got


def test_fix2_run_grows_a_record_set(rfx, prm):
    """a user of the DynPacked call (rfx_dev_fix2_run)"""
    from reflexiv_amd.api import DynPacked
    d = rfx.dyn_pack(host(records(np.random.default_rng(1), LENGTHS)))
    grows(rfx, "fix2_run", lambda o: rfx.fix2_run(d, 2, prm, out=o), DynPacked(1, 1), lambda r: (r.n, r.words))


def test_dedup_dev_grows_a_contig_set(rfx):
    """a user of the ContigsPacked call (rfx_dev_dedup_contigs)"""
    from reflexiv_amd.api import ContigsPacked
    rng = np.random.default_rng(2)
    d = rfx.contigs_pack([M.rand_seq(rng, L) for L in LENGTHS])
    rounds = []

    def call(o):
        out, rn = rfx.dedup_dev(d, out=o)
        rounds.append(rn)
        return out
    grows(rfx, "dedup_dev", call, ContigsPacked(1, 1), lambda r: (r.n, r.words))
    assert rounds[0] == rounds[1]


def test_fix_contig_ends_grows_the_records_and_the_kmers_each_on_its_own(rfx, prm):
    import torch
    from reflexiv_amd.api import DynPacked
    b = rfx.fix_binarize(*upload(lines(contig_rows(np.random.default_rng(3), 4, MAX_K))), prm)
    kmers = []

    def call(o, d_kmers=None):
        out, dk, nk = rfx.fix_contig_ends(b, prm, out=o, d_kmers=d_kmers)
        kmers.append(dk[:nk].cpu().tolist())
        return out
    want, _ = grows(rfx, "fix_contig_ends", lambda o: call(o, None if o is None else torch.empty(1, dtype=torch.int64, device="cuda")), DynPacked(1, 1),
                    lambda r: (r.n, r.words))
    assert kmers[0] == kmers[1] and len(kmers[0]) > 1
    # the k-mers alone short: the set that was large enough comes back as it is
    roomy = DynPacked(want.n, want.words)
    assert call(roomy, torch.empty(1, dtype=torch.int64, device="cuda")) is roomy and kmers[2] == kmers[0]
    same(want, roomy, "fix_contig_ends, short k-mers only")


def test_fix2_contigs_grows_the_set_and_left_right_with_it(rfx, prm):
    from reflexiv_amd.api import ContigsPacked
    d = rfx.dyn_pack(host(records(np.random.default_rng(4), LENGTHS)))
    ends = []

    def call(o):
        c, dl, dr = rfx.fix2_contigs(d, prm, out=o)
        assert dl.numel() >= c.n and dr.numel() >= c.n
        ends.append((dl[:c.n].cpu().tolist(), dr[:c.n].cpu().tolist()))
        return c
    grows(rfx, "fix2_contigs", call, ContigsPacked(1, 1), lambda r: (r.n, r.words))
    assert ends[0] == ends[1]


def test_map_ends_grows_the_hits(rfx, mapped):
    from reflexiv_amd.api import MapHits
    c, dl, dr, reads, _ = mapped
    grows(rfx, "map_ends", lambda o: rfx.map_ends(c, dl, dr, *reads, out=o), MapHits(1), lambda r: (r.n,))


def test_endext_consensus_grows_both_sets(rfx, mapped):
    from reflexiv_amd.api import EndextConsensus
    c, dl, dr, _, rows = mapped
    grows(rfx, "endext_consensus", lambda o: rfx.endext_consensus(c, dl, dr, *rows, out=o), EndextConsensus(1, 1, 1),
          lambda r: (r.left.n, r.right.n, r.left.words, r.right.words))


def test_endext_contigs_grows_the_set(rfx, mapped):
    from reflexiv_amd.api import EndextSet
    c, dl, dr, _, rows = mapped
    cons = rfx.endext_consensus(c, dl, dr, *rows)
    grows(rfx, "endext_contigs", lambda o: rfx.endext_contigs(c, dl, dr, cons, MAX_K, out=o), EndextSet(1, 1), lambda r: (r.n, r.set.words))


@pytest.fixture(scope="module")
def rows07():
    """four rows of 07EndExtend"""
    return upload(lines(genome_rows(np.random.default_rng(5), 4, MAX_K)))


def test_ext_from_text_grows_the_set(rfx, prm, rows07):
    from reflexiv_amd.api import EndextSet
    grows(rfx, "ext_from_text", lambda o: rfx.ext_from_text(*rows07, prm, out=o), EndextSet(1, 1), lambda r: (r.n, r.set.words))


def test_ext_contig_ends_grows_the_records_and_the_kmers_each_on_its_own(rfx, prm, rows07):
    import torch
    from reflexiv_amd.api import DynPacked
    s = rfx.ext_from_text(*rows07, prm)
    kmers = []

    def call(o, d_kmers=None):
        out, dk, nk = rfx.ext_contig_ends(s, prm, out=o, d_kmers=d_kmers)
        kmers.append(dk[:nk].cpu().tolist())
        return out
    want, _ = grows(rfx, "ext_contig_ends", lambda o: call(o, None if o is None else torch.empty(1, dtype=torch.int64, device="cuda")), DynPacked(1, 1),
                    lambda r: (r.n, r.words))
    assert kmers[0] == kmers[1] and len(kmers[0]) > 1
    roomy = DynPacked(want.n, want.words)
    assert call(roomy, torch.empty(1, dtype=torch.int64, device="cuda")) is roomy and kmers[2] == kmers[0]
    same(want, roomy, "ext_contig_ends, short k-mers only")
