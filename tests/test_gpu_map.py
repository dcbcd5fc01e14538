"""Reads onto the contig ends (rfx_dev_map_ends, rfx_dev_map_to_text, rfx_map_text) on the device against the
brute-force string model (tests/map_model.py, which IS the stage's definition and which test_map_model.py ties to its consumer): the
hits field by field and the text byte for byte, through all three entry points; read lengths and overlaps at every edge the rules
name; mismatches at the limit, on word edges and inside the seed; the seed at every residue of a word in the read and in the contig;
every target shape; N and junk behind a read's length; counts around a workgroup; the resident chains into the end extension and the
`mapping` sub-command; the text-buffer rule at every cap; the argument, capacity and limit contracts; and all of it again with every
allocation poisoned."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import endext_model as E
from tests import fixing2_model as F2
from tests import map_model as M
from tests.test_gpu_dedup_packed import CODE
from tests.test_gpu_dynamic_packed import FILL, OK, E_ARG, E_CAP, E_LIMIT
from tests.test_gpu_endext import dev_contigs
from tests.test_gpu_fixing import lines
from tests.test_gpu_ksort import upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)


@pytest.fixture(scope="module")
def rfx():
    import reflexiv_amd
    r = reflexiv_amd.Reflexiv()
    yield r
    r.close()


def pack_reads(reads, wpr=None, junk=None):
    """the 2-bit read store as numpy: (words uint64 [n, wpr], lengths uint32).  junk (an rng): every bit behind a read's last base,
    in its last word and in the words behind it, is random"""
    n = len(reads)
    wpr = wpr or max([1] + [(len(r) + 31) // 32 for r in reads])
    codes = (junk.integers(0, 4, (max(n, 1), wpr * 32)) if junk is not None else np.zeros((max(n, 1), wpr * 32))).astype(np.uint64)
    for i, r in enumerate(reads):
        codes[i, :len(r)] = CODE[np.frombuffer(r.encode(), np.uint8)]
    words = np.bitwise_or.reduce(codes.reshape(max(n, 1), wpr, 32) << SHIFTS, axis=2)
    return words, np.array([len(r) for r in reads] + [0] * (n == 0), np.uint32), wpr


def dev_reads(reads, wpr=None, junk=None):
    import torch
    words, lens, wpr = pack_reads(reads, wpr, junk)
    d = torch.from_numpy(words.view(np.int64).reshape(-1).copy()).cuda(), torch.from_numpy(lens.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    return d[0], d[1], wpr


def check(rfx, contigs, reads, tag, junk=None, wpr=None, at_least=0, **prm):
    """the three entry points on one input against the string model -> (the model's hits, the text)"""
    hs = M.hits(contigs, reads, **{**M.DEFAULTS, **prm})
    assert len(hs) >= at_least, (tag, len(hs))
    c, dl, dr = dev_contigs(rfx, contigs)
    dw, dn, wpr = dev_reads(reads, wpr, junk)
    p = rfx.map_params(**prm)
    got = rfx.map_ends(c, dl, dr, dw, dn, len(reads), wpr, p)
    assert rfx.last_call_ms > 0
    want, g = M.fields(hs), got.host()
    assert got.n == len(hs), (tag, got.n, len(hs))
    for a in got.ARRAYS:
        assert np.array_equal(g[a], want[a]), (tag, a, g[a].tolist()[:12], want[a].tolist()[:12])
    assert got.seed == p.seed
    t, ln, off = rfx.map_to_text(c, dl, dr, dw, dn, wpr, got)
    rows = [M.row_of(h) + "\n" for h in hs]
    text = bytes(t[:ln].cpu().numpy()).decode()
    assert text == "".join(rows), (tag, "text")
    assert off.cpu().tolist() == [0] + list(np.cumsum([len(r) for r in rows])), (tag, "row offsets")
    assert rfx.map_text(M.contig_text(contigs).encode(), [r.encode() for r in reads], p).decode() == text, (tag, "host form")
    return hs, text


def make_contigs(rng, lengths):
    return [(f"Contig_{L}_{int(rng.integers(-3, 4))}_{int(rng.integers(-3, 4))}_{i}", M.rand_seq(rng, L)) for i, L in enumerate(lengths)]


def over_left(rng, bases, n, over):
    """a read of n bases that hangs `over` bases over the left end"""
    return M.rand_seq(rng, over) + bases[:n - over]


def over_right(rng, bases, n, over):
    return bases[max(0, len(bases) - (n - over)):] + M.rand_seq(rng, over)


def both(reads):
    return [x for r in reads for x in (r, M.revcomp(M.norm(r)))]


def flip(s, at):
    return s[:at] + "ACGT"[("ACGT".index(s[at]) + 1) % 4] + s[at + 1:]


# ---- 1. read lengths and overlaps ------------------------------------------------------------------------------------------------------
def test_read_lengths_and_overlaps_at_every_edge(rfx):
    """read lengths 1, seed - 1, seed, seed + 1 (the shortest that can hit), 31..33, 63..65, 150, 151 and 32 words_per_read; overhang
    1 and the largest that leaves min_overlap; v at min_overlap and one below"""
    rng = np.random.default_rng(1)
    contigs = make_contigs(rng, [100, 450])
    reads = []
    for n in (1, 20, 21, 22, 31, 32, 33, 63, 64, 65, 150, 151, 160):
        for over in (1, n - 31, n - 30, n - 21, n - 20):
            if 1 <= over < n:
                reads += [over_left(rng, contigs[0][1], n, over), over_right(rng, contigs[1][1], n, over),
                          over_right(rng, contigs[0][1], n, over), over_left(rng, contigs[1][1], n, over)]
    reads = both(reads) + ["A", "ACGT" * 5, contigs[0][1][:21], contigs[0][1][:22]]
    hs, _ = check(rfx, contigs, reads, "lengths", wpr=5, at_least=100)
    assert {31, 32} <= {h[4] for h in hs} and 30 not in {h[4] for h in hs} and {1, 119, 120, 129} <= {h[6] for h in hs}
    hs, _ = check(rfx, contigs, reads, "lengths, min_overlap = seed", wpr=5, at_least=100, min_overlap=21)
    assert 21 in {h[4] for h in hs} and 22 in {len(h[8]) for h in hs} and 21 not in {len(h[8]) for h in hs}


# ---- 2. mismatches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_mismatch", (0, 2, 3))
def test_mismatches_at_the_limit_on_word_edges_and_inside_the_seed(rfx, max_mismatch):
    rng = np.random.default_rng(2)
    contigs = make_contigs(rng, [130, 450])
    reads = []
    over, n = 37, 150
    # left end of the whole-contig target: overlap index t is read base 37 + t and contig base t.  The last base of the overlap, the
    # word edges of the contig (31 | 32, 63 | 64) and of the read (63 | 64 = t 26 | 27, 95 | 96 = t 58 | 59)
    base = over_left(rng, contigs[0][1], n, over)
    v = n - over
    spots = [v - 1, 32, 31, 27, 26, 64, 63, 58, 59]
    for k in range(5):
        for rot in range(len(spots)):
            r = base
            for t in (spots[rot:] + spots[:rot])[:k]:
                r = flip(r, over + t)
            reads.append(r)
    reads += [flip(base, over + t) for t in (0, 5, 20)]            # inside the seed: no row
    # right end of a 200-base target: overlap index t counts back from the contig's last base
    base = over_right(rng, contigs[1][1], n, over)
    for k in range(5):
        for rot in range(len(spots)):
            r = base
            for t in (spots[rot:] + spots[:rot])[:k]:
                r = flip(r, v - 1 - t)
            reads.append(r)
    reads += [flip(base, v - 1 - t) for t in (0, 5, 20)]
    hs, _ = check(rfx, contigs, both(reads), ("mismatches", max_mismatch), max_mismatch=max_mismatch)
    # nine reads for each number of mismatches 0..4, two ends, two strands: those of max_mismatch or fewer give a row, no other does
    assert len(hs) == 2 * 2 * 9 * (max_mismatch + 1)


# ---- 3. placement and strand -------------------------------------------------------------------------------------------------------------
def test_the_seed_at_every_residue_of_a_word_in_the_read_and_in_the_contig(rfx):
    rng = np.random.default_rng(3)
    contigs = make_contigs(rng, [120] + list(range(400, 432)))
    reads = []
    for over in range(1, 41):                                      # every read offset residue mod 32, on a whole target and on an -L
        reads += [over_left(rng, contigs[0][1], 100, over), over_left(rng, contigs[1 + over % 32][1], 100, over)]
    for i in range(1, 33):                                         # the right end of contigs of 400..431 bases, the seed anywhere in the read
        reads += [over_right(rng, contigs[i][1], 100, 1 + (7 * i) % 60), over_right(rng, contigs[i][1], 150, 40 + i)]
    hs, _ = check(rfx, contigs, both(reads), "residues", at_least=4 * 72)
    assert {h[3] % 32 for h in hs if not h[1] & 1} == set(range(32)) == {h[3] % 32 for h in hs if h[1] & 1}
    assert {0, 1} == {h[2] for h in hs}


def test_shared_seeds_palindromes_two_ends_in_one_read_and_tandem_repeats(rfx):
    rng = np.random.default_rng(4)
    pal = "ACGTAGGCTA" + M.revcomp("ACGTAGGCTA")
    shared = M.rand_seq(rng, 100)
    unit = M.rand_seq(rng, 25)
    contigs = [pal + M.rand_seq(rng, 60),                           # 0: a palindromic 20-base seed at the left end
               M.rand_seq(rng, 60) + pal,                           # 1: and the same seed at a right end
               shared + M.rand_seq(rng, 50), shared + M.rand_seq(rng, 400),      # 2, 3: the same 100 bases at two left ends
               shared[:40] + M.rand_seq(rng, 90),                   # 4: the same seed, another target behind it
               M.rand_seq(rng, 450), M.rand_seq(rng, 450),          # 5, 6: a read over the -R of one and the -L of the other
               unit + unit + M.rand_seq(rng, 40)]                   # 7: a tandem repeat at the left end
    contigs = [(f"Contig_{len(b)}_{i}_{-i}_{i}", b) for i, b in enumerate(contigs)]
    reads = ["GG" + contigs[0][1][:60], contigs[1][1][20:] + "TT", M.rand_seq(rng, 30) + shared[:70], M.rand_seq(rng, 9) + shared[:35],
             contigs[5][1][-50:] + contigs[6][1][:50], "C" + unit * 3, "C" + unit * 4]
    for seed, mm in ((20, 2), (21, 2), (20, 31)):
        hs, _ = check(rfx, contigs, both(reads), ("special", seed, mm), at_least=10, seed=seed, max_mismatch=mm)
        by = {}
        for h in hs:
            by.setdefault(h[0], []).append(h[1:5])
        assert {e for e, _, _, _ in by[4]} == ({4, 6, 8} if mm == 31 else {4, 6})      # the third target too, once the mismatches are allowed
        assert {e for e, _, _, _ in by[6]} == {4, 6, 8} and {e for e, _, _, _ in by[8]} == {11, 12}
        assert (0, 0, 2, 60) in by[0] and 3 in {e for e, _, _, _ in by[2]}
        if mm == 31:
            assert [x for x in by[10] if x[0] == 14 and x[1] == 0] == [(14, 0, 1, 75), (14, 0, 26, 50)]


# ---- 4. contig and read lengths ----------------------------------------------------------------------------------------------------------
def test_every_target_shape(rfx):
    """contigs of 62, 199, 200, 399, 400, 401 and 3,000 bases; a whole-contig target shorter than the read (the both-ends rule) and
    one exactly n - 1 long; reads longer than 200 on -L and -R targets (a clip at the far end)"""
    rng = np.random.default_rng(5)
    contigs = make_contigs(rng, [62, 199, 200, 399, 400, 401, 3000, 20, 21])
    reads = []
    for _, b in contigs:
        for n, over in ((100, 1), (100, 40), (150, 69), (260, 40), (260, 10), (461, 30)):
            reads += [over_left(rng, b, n, over), over_right(rng, b, n, over)]
    short = contigs[0][1]
    reads += [M.rand_seq(rng, 20) + short + M.rand_seq(rng, 20), M.rand_seq(rng, 1) + short, short + M.rand_seq(rng, 1),
              M.rand_seq(rng, 1) + short + M.rand_seq(rng, 1)]
    hs, text = check(rfx, contigs, both(reads), "shapes", at_least=100)
    two = {h[7][-2:] for h in hs if h[5] > 0}
    assert two == {"-L", "-R"} and not any(h[5] for h in hs if h[7][-2] != "-")
    assert {h[9] for h in hs} == {62, 199, 200, 399}
    n = len(reads)
    got = {h[0] // 2: h for h in hs if h[0] % 2 == 0}
    assert n - 4 not in got and n - 1 not in got and got[n - 3][1:5] == (0, 0, 1, 62) and got[n - 2][1] == 1
    assert "\t40S200M20S\t" in text and "\t20S200M40S\t" in text and "S62M\t" in text


# ---- 5. N, junk behind a read's length, poisoned allocations -----------------------------------------------------------------------------
def test_n_in_reads_and_junk_behind_each_reads_length(rfx):
    rng = np.random.default_rng(6)
    contigs = make_contigs(rng, [90, 450, 130])
    reads = []
    for n in (33, 60, 64, 65, 95, 96, 97, 100, 127, 128):
        for i, (_, b) in enumerate(contigs):
            l, r = list(over_left(rng, b, n, 1 + (n + i) % 30)), list(over_right(rng, b, n, 2 + (n + 2 * i) % 30))
            l[int(rng.integers(0, len(l)))] = "N"
            r[int(rng.integers(0, len(r)))] = "n"
            reads += ["".join(l), "".join(r)]
    t_contig = contigs[0][1][:10] + "T" + contigs[0][1][11:]
    contigs[0] = (contigs[0][0], t_contig)
    reads.append("GGG" + t_contig[:10] + "N" + t_contig[11:70])     # an N where the contig has a T: a match, seed included
    reads = both(reads)
    want = check(rfx, contigs, reads, "N, clean", wpr=4, at_least=40)
    assert any(h[0] == len(reads) - 2 for h in want[0])
    assert check(rfx, contigs, reads, "N, junk", wpr=4, junk=rng, at_least=40) == want
    assert check(rfx, contigs, reads, "N, junk, wider", wpr=7, junk=rng, at_least=40) == want


def test_the_stage_holds_with_every_allocation_poisoned():
    """RFX_POISON=7 (rfx_internal.h): every scratch allocation is filled with 0xA5 before the library uses it, so a kernel that
    relied on zeroed memory fails the checks above.  A child process: the mask is read once per process."""
    env = dict(os.environ, RFX_POISON="7")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", here, "-k",
                        "not poisoned and not sub_command and not counts and not outside"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ---- 6. counts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 2, 255, 256, 257))
def test_contig_counts_around_a_block(rfx, n):
    rng = np.random.default_rng(100 + n)
    contigs = make_contigs(rng, [int(x) for x in rng.integers(62, 140, n)] if n < 200 else [int(x) for x in rng.choice((70, 410, 95), n)])
    reads = [M.rand_seq(rng, 100) for _ in range(8)]
    for i in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
        reads += [over_left(rng, contigs[i][1], 100, 33), over_right(rng, contigs[i][1], 100, 44)]
    check(rfx, contigs, both(reads), ("contigs", n), at_least=min(n, 5) * 4)


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257, 513))
def test_read_counts_around_a_wave_and_a_workgroups_share(rfx, n):
    rng = np.random.default_rng(200 + n)
    contigs = make_contigs(rng, [90, 450, 130])
    reads = []
    for i in range(n):
        b = contigs[i % 3][1]
        reads.append(M.rand_seq(rng, 80) if i % 5 == 4 else over_left(rng, b, 70 + i % 60, 1 + i % 37) if i % 2 else over_right(rng, b, 70 + i % 60, 1 + i % 37))
        if i % 4 == 0:
            reads[-1] = M.revcomp(reads[-1])
    hs, _ = check(rfx, contigs, reads, ("reads", n), at_least=n // 2)
    if n:
        assert hs == [] or max(h[0] for h in hs) >= n - 3


def seed_values(contigs, seed):
    """the table's keys as the kernels form them: the end seeds and their reverse complements as 2 * seed bit numbers"""
    out = set()
    for _, b in contigs:
        if len(b) >= seed:
            for s in (b[:seed], b[len(b) - seed:]):
                for x in (s, M.revcomp(s)):
                    out.add(int("".join(str("ACGT".index(ch)) for ch in x), 4))
    return np.array(sorted(out), np.uint64)


def test_windows_the_filters_pass_and_the_table_rejects(rfx):
    """3,000 random reads against 257 contigs: 1,028 keys in the LDS filter's 2^18 bits pass about one window in 255, so some thousand
    windows go on to the second filter (2^24 bits) and a few of those to the table.  Then windows CRAFTED from both hashes (the two
    constants of rfx_endmap.hip, restated here: with other constants the crafted reads would merely stop reaching the table) that pass
    both filters and are no key: the table search finds nothing for them, and the reads that do map are found among them"""
    rng = np.random.default_rng(7)
    contigs = make_contigs(rng, [int(x) for x in rng.choice((70, 410, 95, 130), 257)])
    keys = seed_values(contigs, 21)
    bits1, bits2 = np.zeros(1 << 18, bool), np.zeros(1 << 24, bool)
    h1 = lambda v: (v * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - 18)       # noqa: E731  (uint64 arithmetic wraps, as the kernel's)
    h2 = lambda v: (v * np.uint64(0xC2B2AE3D27D4EB4F)) >> np.uint64(64 - 24)       # noqa: E731
    bits1[h1(keys)] = True
    bits2[h2(keys)] = True
    crafted = []
    for _ in range(40):
        v = rng.integers(0, 1 << 42, 2_000_000).astype(np.uint64)
        v = v[bits1[h1(v)]]
        crafted += [int(x) for x in v[bits2[h2(v)]] if int(x) not in set(keys.tolist())]
        if len(crafted) >= 4:
            break
    assert len(crafted) >= 2
    reads = [M.rand_seq(rng, 150) for _ in range(3000)]
    for j, v in enumerate(crafted[:8]):
        mer = "".join("ACGT"[(v >> (2 * (20 - t))) & 3] for t in range(21))
        reads[100 + 3 * j] = M.rand_seq(rng, 17 + j) + mer + M.rand_seq(rng, 60)
        reads[101 + 3 * j] = M.revcomp(reads[100 + 3 * j])
    for i in range(0, 257, 8):
        reads[300 + 10 * i] = over_left(rng, contigs[i][1], 150, 50)
        reads[301 + 10 * i] = M.revcomp(over_right(rng, contigs[i][1], 150, 60))
    c, dl, dr = dev_contigs(rfx, contigs)
    dw, dn, wpr = dev_reads(reads)
    hs = M.hits(contigs, reads)
    got = rfx.map_ends(c, dl, dr, dw, dn, len(reads), wpr)
    want, g = M.fields(hs), got.host()
    assert got.n == len(hs) >= 66
    for a in got.ARRAYS:
        assert np.array_equal(g[a], want[a]), a
    t, ln, _ = rfx.map_to_text(c, dl, dr, dw, dn, wpr, got)
    assert bytes(t[:ln].cpu().numpy()).decode() == "".join(M.row_of(h) + "\n" for h in hs)


# ---- 7. chains ---------------------------------------------------------------------------------------------------------------------------
def chain_text(rfx, c, dl, dr, reads, max_k):
    """map_ends -> map_to_text -> endext_consensus -> endext_contigs -> endext_to_text, nothing on the host -> (rows, 07EndExtend)"""
    dw, dn, wpr = dev_reads(reads)
    hits = rfx.map_ends(c, dl, dr, dw, dn, len(reads), wpr)
    t, ln, off = rfx.map_to_text(c, dl, dr, dw, dn, wpr, hits)
    cons = rfx.endext_consensus(c, dl, dr, t, off)
    o, n = rfx.endext_to_text(rfx.endext_contigs(c, dl, dr, cons, max_k))
    return bytes(t[:ln].cpu().numpy()).decode(), bytes(o[:n].cpu().numpy()).decode()


@pytest.fixture(scope="module")
def planted():
    genome, spans, contigs, reads = M.planted_case()
    rows = M.rows(contigs, reads)
    return contigs, reads, rows, E.run_text(M.contig_text(contigs), rows, 31)


def test_the_resident_chain_on_the_planted_genome_equals_the_string_models(rfx, planted):
    contigs, reads, rows, want = planted
    c, dl, dr = dev_contigs(rfx, contigs)
    got_rows, got = chain_text(rfx, c, dl, dr, reads, 31)
    assert got_rows == "".join(r + "\n" for r in rows) and len(rows) > 100
    assert got == want and want.count("\n") == len(contigs)
    assert rfx.map_text(M.contig_text(contigs).encode(), [r.encode() for r in reads]).decode() == got_rows
    assert rfx.endext_text(M.contig_text(contigs).encode(), got_rows.encode(), 31).decode() == want


def test_fix2_contigs_feed_the_chain_with_no_text_in_between(rfx):
    """rows of 04Fixing -> rfx_dev_fix2_* -> the contigs in HBM -> the chain, with reads simulated from the contigs' ends"""
    z2 = np.load(os.path.join(ROOT, "tests", "golden", "fixing2_vectors.npz"))
    p, P, rows = F2.load_case(z2, "fix_k41_P7_s2_M3")[:3]
    prm = rfx.fix_params(p["max_k"], scramble=p["scramble"], max_iteration=p["max_iteration"])
    c, dl, dr = rfx.fix2_contigs(rfx.fix2_run(rfx.fix2_binarize(*upload(lines(rows))), P, prm), prm)
    t, n = rfx.fix2_to_text(c, dl, dr)
    ctext = bytes(t[:n].cpu().numpy()).decode()
    contigs = E.contigs_of_text(ctext)
    assert len(contigs) == c.n > 0
    rng = np.random.default_rng(8)
    reads = []
    for _, b in contigs[:40]:
        reads += [over_left(rng, b, 100, 45), over_left(rng, b, 150, 70), over_right(rng, b, 100, 30), over_right(rng, b, 150, 90)]
    reads = both(reads)
    want_rows = M.rows(contigs, reads)
    got_rows, got = chain_text(rfx, c, dl, dr, reads, p["max_k"])
    assert got_rows == "".join(r + "\n" for r in want_rows) and len(want_rows) >= len(reads) // 2
    assert got == E.run_text(ctext, want_rows, p["max_k"])
    assert rfx.map_text(ctext.encode(), [r.encode() for r in reads]).decode() == got_rows


def test_the_mapping_sub_command_writes_the_chains_text_and_rows(planted, tmp_path):
    contigs, reads, rows, want = planted
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    d = tmp_path / "05FixingAgain"
    d.mkdir()
    (d / "part-00000.csv").write_text(M.contig_text(contigs))
    fq, out, rows_out = tmp_path / "reads.fq", tmp_path / "out", tmp_path / "rows.tsv"
    fq.write_text("".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)))
    r = subprocess.run([exe, "mapping", "-kmerc", str(d), "-fastq", str(fq), "-klist", "23,31", "-outfile", str(out), "-rowsout", str(rows_out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = out / "Assembly_intermediate" / "07EndExtend"
    assert (d / "part-00000.csv").read_text() == want and (d / "_SUCCESS").exists()
    assert rows_out.read_text() == "".join(x + "\n" for x in rows)
    r = subprocess.run([exe, "mapping"], capture_output=True, text=True)
    assert r.returncode != 0 and "-kmerc" in r.stderr and "-fastq" in r.stderr


def test_reads_to_contigs_with_no_program_outside_this_repository(rfx, planted, tmp_path):
    """reflexiv_host mapping, extend and extend2, then the de-duplication, on the planted genome: every contig that comes out is a piece
    of the genome, and together they close every gap between the planted contigs (each gap is at most 120 bases and a read of 150
    hangs up to 119 over an end, so the two extensions into a gap meet)"""
    contigs, reads, rows, want = planted
    genome, spans = M.planted_case()[:2]
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    d = tmp_path / "05FixingAgain"
    d.mkdir()
    (d / "part-00000.csv").write_text(M.contig_text(contigs))
    fq, out = tmp_path / "reads.fq", tmp_path / "out"
    fq.write_text("".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)))
    ai = out / "Assembly_intermediate"
    for cmd, src in (("mapping", d), ("extend", ai / "07EndExtend"), ("extend2", ai / "08Extend")):
        r = subprocess.run([exe, cmd, "-kmerc", str(src)] + (["-fastq", str(fq)] if cmd == "mapping" else []) +
                           ["-klist", "23,31", "-partition", "2", "-outfile", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, (cmd, r.stderr)
    final = [x.split(",")[1] for x in (ai / "09ExtendAgain" / "part-00000.csv").read_text().splitlines()]
    kept = rfx.dedup_contigs(final, min_contig=62)[0]
    assert 0 < len(kept) <= len(final)
    covered = np.zeros(len(genome), bool)
    for c in kept:
        assert c in genome or M.revcomp(c) in genome, len(c)
        at = genome.find(c) if c in genome else genome.find(M.revcomp(c))
        covered[at:at + len(c)] = True
    assert covered[spans[0][0]:spans[-1][1]].all() and covered.sum() > sum(e - s for s, e in spans)


# ---- 8. the text-buffer rule -------------------------------------------------------------------------------------------------------------
def small_input(rfx):
    rng = np.random.default_rng(9)
    contigs = make_contigs(rng, [70, 410])
    reads = [over_left(rng, contigs[0][1], 45, 12), M.revcomp(over_right(rng, contigs[1][1], 50, 15)), M.rand_seq(rng, 40),
             over_left(rng, contigs[1][1], 33, 2)]
    return contigs, reads


def test_the_text_buffer_rule_at_every_cap_with_an_unaligned_destination(rfx):
    import torch
    contigs, reads = small_input(rfx)
    c, dl, dr = dev_contigs(rfx, contigs)
    dw, dn, wpr = dev_reads(reads)
    hits = rfx.map_ends(c, dl, dr, dw, dn, len(reads), wpr)
    want = np.frombuffer("".join(r + "\n" for r in M.rows(contigs, reads)).encode(), np.uint8)
    n = len(want)
    assert hits.n == 3 and 150 < n < 400
    ci, hi = c._c(), hits._c()
    off = torch.empty(hits.n + 1, dtype=torch.int64, device="cuda")
    for cap in list(range(n + 1)) + [n + 5]:
        shift = 1 + (7 * cap) % 15
        buf = torch.full((n + 96,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ln = C.c_int64(-77)
        st = rfx.L.rfx_dev_map_to_text(rfx.ctx, C.byref(ci), dl.data_ptr(), dr.data_ptr(), dw.data_ptr(), dn.data_ptr(), wpr, C.byref(hi),
                                       buf.data_ptr() + 32 + shift, cap, C.addressof(ln), off.data_ptr(), hits.n + 1)
        got = buf.cpu().numpy()
        lim = min(cap, n)
        assert st == (OK if cap >= n else E_CAP) and ln.value == n, (cap, st)
        assert np.array_equal(got[32 + shift:32 + shift + lim], want[:lim]), cap
        assert (got[:32 + shift] == FILL).all() and (got[32 + shift + lim:] == FILL).all(), cap
    # the host form with a short buffer writes nothing
    ct = M.contig_text(contigs).encode()
    oc, nc = rfx._row_offsets(ct)
    bases = "".join(reads).encode()
    ro = np.zeros(len(reads) + 1, np.int64)
    ro[1:] = np.cumsum([len(r) for r in reads])
    p = rfx.map_params()
    for cap in (0, n - 1, n):
        o, ln = np.full(n + 16, FILL, np.uint8), C.c_int64(0)
        st = rfx.L.rfx_map_text(rfx.ctx, ct, oc.ctypes.data, nc, bases, ro.ctypes.data, len(reads), C.byref(p), o.ctypes.data, cap, C.addressof(ln))
        assert st == (OK if cap >= n else E_CAP) and ln.value == n
        assert (o == FILL).all() if cap < n else (np.array_equal(o[:n], want) and (o[n:] == FILL).all())


# ---- 9. contracts --------------------------------------------------------------------------------------------------------------------------
def poisoned_hits(cap_n):
    import torch
    from reflexiv_amd.api import MapHits
    h = MapHits(cap_n)
    ts = [getattr(h, a) for a in h.ARRAYS]
    for t in ts:
        t.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    return h, ts


def all_untouched(ts):
    import torch
    return all(bool((t.view(torch.uint8) == FILL).all()) for t in ts)


def test_every_refused_argument_leaves_the_outputs_untouched(rfx):
    import torch
    L, ctx = rfx.L, rfx.ctx
    contigs, reads = small_input(rfx)
    c, dl, dr = dev_contigs(rfx, contigs)
    dw, dn, wpr = dev_reads(reads)
    ci = c._c()
    nr = len(reads)
    good = rfx.map_ends(c, dl, dr, dw, dn, nr, wpr)
    h, ts = poisoned_hits(16)
    buf = torch.full((1024,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ln = C.c_int64(-77)
    P = rfx.map_params
    ends = lambda ci_, l, r, w, n_, k, wp, p, ho: L.rfx_dev_map_ends(ctx, ci_, l, r, w, n_, k, wp, p, ho)      # noqa: E731
    A = (C.byref(ci), dl.data_ptr(), dr.data_ptr(), dw.data_ptr(), dn.data_ptr(), nr, wpr)
    # the parameters
    for bad in (P(seed=10), P(seed=32), P(min_overlap=20), P(min_overlap=201), P(max_mismatch=-1), P(max_mismatch=32), P(seed=31, min_overlap=30)):
        assert ends(*A, C.byref(bad), C.byref(h._c())) == E_ARG, (bad.seed, bad.min_overlap, bad.max_mismatch)
    for fine in (P(seed=11, min_overlap=11), P(seed=31, min_overlap=200, max_mismatch=31), P(max_mismatch=0)):
        hh, _ = poisoned_hits(16)
        assert ends(*A, C.byref(fine), C.byref(hh._c())) == OK
    # null pointers, negative counts, words_per_read
    p = C.byref(P())
    for i in (0, 1, 2, 3, 4):
        a = list(A)
        a[i] = None
        assert ends(*a, p, C.byref(h._c())) == E_ARG, i
    assert ends(*A, None, C.byref(h._c())) == E_ARG and ends(*A, p, None) == E_ARG
    assert ends(*A[:5], -1, wpr, p, C.byref(h._c())) == E_ARG and ends(*A[:6], 0, p, C.byref(h._c())) == E_ARG
    for a in h.ARRAYS:
        no = h._c()
        setattr(no, a, None)
        assert ends(*A, p, C.byref(no)) == E_ARG, a
    # a read longer than its words: found by the counting pass
    keep = int(dn[2])
    dn[2] = 32 * wpr + 1
    torch.cuda.synchronize()
    assert ends(*A, p, C.byref(h._c())) == E_ARG and "32 * words_per_read" in rfx.L.rfx_last_error(ctx).decode()
    dn[2] = keep
    # a contig set whose word_off and len disagree; a contig of 2^30 bases with its word_off in step
    for field, at, value in (("len", 1, -1), ("word_off", 0, 1), ("word_off", 2, 0), ("len", 0, 7)):
        t = getattr(c, field)
        keep = int(t[at])
        t[at] = value
        torch.cuda.synchronize()
        assert ends(*A, p, C.byref(h._c())) == E_ARG, (field, at, value)
        t[at] = keep
        torch.cuda.synchronize()
    last = c.n - 1
    keep = int(c.len[last]), int(c.word_off[last + 1])
    c.len[last] = 1 << 30
    c.word_off[last + 1] = int(c.word_off[last]) + (1 << 25)
    torch.cuda.synchronize()
    assert ends(*A, p, C.byref(h._c())) == E_LIMIT
    c.len[last], c.word_off[last + 1] = keep
    torch.cuda.synchronize()
    big = c._c()
    big.n = 1 << 29
    assert ends(C.byref(big), *A[1:], p, C.byref(h._c())) == E_LIMIT and ends(*A[:5], 1 << 31, wpr, p, C.byref(h._c())) == E_LIMIT
    # the text writer: null pointers, hits that map_ends cannot have written, too few row offsets
    gi = good._c()
    text = lambda ci_, l, r, w, n_, wp, hi, b, cap, ln_, o, co: L.rfx_dev_map_to_text(ctx, ci_, l, r, w, n_, wp, hi, b, cap, ln_, o, co)      # noqa: E731
    T = (C.byref(ci), dl.data_ptr(), dr.data_ptr(), dw.data_ptr(), dn.data_ptr(), wpr, C.byref(gi), buf.data_ptr(), 1024, C.addressof(ln), off.data_ptr(), 16)
    for i in (0, 1, 2, 3, 4, 6, 7, 9, 10):
        a = list(T)
        a[i] = None
        assert text(*a) == E_ARG, i
    for i, v in ((5, 0), (8, -1), (11, -1)):
        a = list(T)
        a[i] = v
        assert text(*a) == E_ARG, i
    for field, value in (("seed", 10), ("seed", 32), ("n", -1), ("n", 17)):
        b = good._c()
        setattr(b, field, value)
        assert text(*T[:6], C.byref(b), *T[7:]) == E_ARG, (field, value)
    for a, at, value in (("end", 0, -1), ("end", 0, 4), ("strand", 1, 2), ("strand", 1, -1), ("v", 0, 32), ("v", 2, 0), ("offset", 0, 0), ("offset", 0, 40),
                         ("offset", 1, -1), ("read", 0, -1), ("end", 2, 3)):
        t = getattr(good, a)
        keep = int(t[at])
        t[at] = value
        torch.cuda.synchronize()
        assert text(*T) == E_ARG, (a, at, value)
        t[at] = keep
        torch.cuda.synchronize()
    assert text(*T[:11], good.n) == E_CAP and ln.value > 0
    assert bool((buf == FILL).all()) and bool((off == -1).all())
    ln.value = -77
    # the host form
    ct = M.contig_text(contigs).encode()
    oc, nc = rfx._row_offsets(ct)
    bases = "".join(reads).encode()
    ro = np.zeros(nr + 1, np.int64)
    ro[1:] = np.cumsum([len(r) for r in reads])
    o8 = np.full(64, FILL, np.uint8)
    host = lambda ct_, oc_, nc_, b, ro_, nr_, p_, o, cap, ln_: L.rfx_map_text(ctx, ct_, oc_, nc_, b, ro_, nr_, p_, o, cap, ln_)      # noqa: E731
    H = (ct, oc.ctypes.data, nc, bases, ro.ctypes.data, nr, p, o8.ctypes.data, 64, C.addressof(ln))
    for i in (0, 1, 3, 4, 6, 7, 9):
        a = list(H)
        a[i] = None
        assert host(*a) == E_ARG, i
    assert host(*H[:6], C.byref(P(seed=9)), *H[7:]) == E_ARG and host(*H[:2], -1, *H[3:]) == E_ARG and host(*H[:5], -1, *H[6:]) == E_ARG
    assert host(*H[:8], -1, H[9]) == E_ARG
    assert host(*H[:2], 1 << 29, *H[3:]) == E_LIMIT and host(*H[:5], 1 << 31, *H[6:]) == E_LIMIT
    for bad in ("Contig_5_0_0_0,ACGT\n", "Contig_4_0_0_1,ACGT\n", "Contig_4_0_0_0,ACGN\n"):
        b = bad.encode()
        ob, nb = rfx._row_offsets(b)
        assert host(b, ob.ctypes.data, nb, *H[3:]) == E_ARG, bad
    assert (o8 == FILL).all() and all_untouched(ts) and ln.value == -77


def test_every_capacity_one_short_and_the_empty_inputs(rfx):
    import torch
    L, ctx = rfx.L, rfx.ctx
    contigs, reads = small_input(rfx)
    c, dl, dr = dev_contigs(rfx, contigs)
    dw, dn, wpr = dev_reads(reads)
    ci, p = c._c(), rfx.map_params()
    call = lambda ho, cc=ci, n=len(reads): L.rfx_dev_map_ends(ctx, C.byref(cc), dl.data_ptr(), dr.data_ptr(), dw.data_ptr(), dn.data_ptr(), n, wpr, C.byref(p), C.byref(ho))   # noqa: E731
    h, ts = poisoned_hits(3)
    ho = h._c()
    assert call(ho) == OK and (int(ho.n), int(ho.need_n), int(ho.seed)) == (3, 3, 21) and not all_untouched(ts)
    h, ts = poisoned_hits(2)
    ho = h._c()
    ho.n = -77
    assert call(ho) == E_CAP and (int(ho.n), int(ho.need_n)) == (-77, 3) and all_untouched(ts)
    # no contigs, no reads, neither: valid, no rows, an empty text with one row offset
    empty = rfx.contigs_pack([])
    for cc, n in ((empty._c(), len(reads)), (ci, 0), (empty._c(), 0)):
        h, ts = poisoned_hits(2)
        ho = h._c()
        ho.n = -77
        assert call(ho, cc, n) == OK and (int(ho.n), int(ho.need_n)) == (0, 0) and all_untouched(ts)
        buf = torch.full((64,), FILL, dtype=torch.uint8, device="cuda")
        off = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ln = C.c_int64(-77)
        assert L.rfx_dev_map_to_text(ctx, C.byref(cc), dl.data_ptr(), dr.data_ptr(), dw.data_ptr(), dn.data_ptr(), wpr, C.byref(ho), buf.data_ptr(), 64,
                                     C.addressof(ln), off.data_ptr(), 1) == OK
        assert ln.value == 0 and bool((buf == FILL).all()) and off.cpu().tolist() == [0, -1, -1, -1]
    assert rfx.map_text(b"", [r.encode() for r in reads]) == b"" and rfx.map_text(M.contig_text(contigs).encode(), []) == b""
    assert rfx.map_text(b"", []) == b""
