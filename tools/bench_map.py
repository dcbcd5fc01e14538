"""dev helper / bench block: reads onto the contig ends (the front half of the Mapping stage).  Input: the 10,000
contigs (200 to 1,800 bases) of tools/bench_endext.py's input as a packed set in HBM, and --reads (2,000,000) reads of 150 bases
synthesized from them on the host: a window of 150 bases at a uniform position of (150 random bases || contig || 150 random bases) of
a uniform contig, every second one reverse-complemented, one base in 100 replaced -- so a read hangs over an end, lies inside its
contig or misses it, as the reads of an assembly do.  One warm-up, then --runs runs of rfx_dev_map_ends and rfx_dev_map_to_text, each
timed inside the C ABI (Reflexiv.last_call_ms), and of the host form rfx_map_text on the first --host-reads (200,000) reads (its uploads
and copy back included); the median and the spread of each.  The tool asserts that the host form's text is the head of the device
chain's.  It also MEASURES, on the host with the kernel's own hash, what share of the windows of the first --sample (20,000) reads pass
the LDS filter and what share of those the table rejects.  Prints one JSON object; "kernel_bytes" in it gives the algorithmic bytes of
ONE launch of each kernel (the scan: the read store once plus the hits).  For the per-kernel times run it under `rocprofv3
--kernel-trace --stats -- python tools/bench_map.py --runs 1` (no counters in that run), then `python tools/bench_map.py --join STATS
RESULT.json`."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksort import stats  # noqa: E402
from bench_fixing import join  # noqa: E402
from bench_endext import synthesize  # noqa: E402

READ = 150
WPR = 5
SHIFTS = np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)
CODE = np.full(256, 3, np.uint8)
CODE[ord("A")], CODE[ord("C")], CODE[ord("G")] = 0, 1, 2
FILTER_BITS, FILTER2_BITS = 18, 24                                # MP_FILTER_BITS and MP_FILTER2_BITS of rfx_endmap.hip, and its two hashes
GOLD, GOLD2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xC2B2AE3D27D4EB4F)


def make_reads(contigs, n, seed):
    """-> base codes uint8 [n, 150]"""
    rng = np.random.default_rng(seed)
    parts, start, length = [], [], []
    at = 0
    for c in contigs:
        parts += [rng.integers(0, 4, READ).astype(np.uint8), CODE[np.frombuffer(c, np.uint8)], rng.integers(0, 4, READ).astype(np.uint8)]
        start.append(at)
        length.append(len(c) + READ)                               # window starts: from 150 bases ahead of the contig to its last base
        at += len(c) + 2 * READ
    g = np.concatenate(parts)
    start, length = np.array(start, np.int64), np.array(length, np.int64)
    which = rng.integers(0, len(contigs), n)
    pos = start[which] + (rng.random(n) * length[which]).astype(np.int64)
    codes = g[pos[:, None] + np.arange(READ)[None, :]]
    noise = rng.random(codes.shape) < 0.01
    codes[noise] = (codes[noise] + rng.integers(1, 4, int(noise.sum())).astype(np.uint8)) & 3
    rc = np.arange(n) % 2 == 1
    codes[rc] = 3 - codes[rc][:, ::-1]
    return codes


def pack(codes):
    """base codes [n, 150] -> words uint64 [n, 5], in pieces (the shifted copy is eight times the codes)"""
    out = np.zeros((len(codes), WPR), np.uint64)
    for b in range(0, len(codes), 100000):
        c = np.zeros((len(codes[b:b + 100000]), WPR * 32), np.uint64)
        c[:, :READ] = codes[b:b + 100000]
        out[b:b + 100000] = np.bitwise_or.reduce(c.reshape(-1, WPR, 32) << SHIFTS, axis=2)
    return out


def filter_rates(contigs, codes, seed_len):
    """the share of the sample's windows that pass the LDS filter, the share that pass the second filter too, and of those the share
    whose value is no seed of the table"""
    mask = np.uint64((1 << (2 * seed_len)) - 1)

    def value(c):                                                  # base codes [m, seed] -> the window values
        v = np.zeros(len(c), np.uint64)
        for j in range(seed_len):
            v = (v << np.uint64(2)) | c[:, j].astype(np.uint64)
        return v
    ends = np.array([x for c in contigs if len(c) >= seed_len for x in (CODE[np.frombuffer(c[:seed_len], np.uint8)], CODE[np.frombuffer(c[-seed_len:], np.uint8)])])
    keys = np.concatenate([value(ends), value(3 - ends[:, ::-1])]) & mask
    h = lambda v: (v * GOLD) >> np.uint64(64 - FILTER_BITS)       # noqa: E731  (uint64 arithmetic wraps, as the kernel's does)
    h2 = lambda v: (v * GOLD2) >> np.uint64(64 - FILTER2_BITS)    # noqa: E731
    bits, bits2 = np.zeros(1 << FILTER_BITS, bool), np.zeros(1 << FILTER2_BITS, bool)
    bits[h(keys)] = True
    bits2[h2(keys)] = True
    win = np.lib.stride_tricks.sliding_window_view(codes, seed_len, axis=1).reshape(-1, seed_len)
    v = value(win)
    passed = bits[h(v)]
    both = v[passed][bits2[h2(v[passed])]]
    in_table = np.isin(both, keys)
    return {"filter_bits_set": int(bits.sum()), "filter_fill": float(bits.mean()), "filter2_fill": float(bits2.mean()), "windows": int(len(v)),
            "filter_pass_rate": float(passed.mean()), "both_filters_pass_rate": float(len(both) / len(v)),
            "table_reject_share_of_both_passed": float(1.0 - in_table.mean()) if len(both) else None}


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--join":
        return join(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=10000)
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--host-reads", type=int, default=200000)
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=24)
    a = ap.parse_args()
    import torch
    import reflexiv_amd
    rfx = reflexiv_amd.Reflexiv()
    contigs, lr, _, _, _ = synthesize(a.contigs, 1, a.seed)
    c = rfx.contigs_pack([x.decode() for x in contigs])
    dl, dr = torch.from_numpy(np.ascontiguousarray(lr[:, 0])).cuda(), torch.from_numpy(np.ascontiguousarray(lr[:, 1])).cuda()
    codes = make_reads(contigs, a.reads, a.seed + 1)
    dw = torch.from_numpy(pack(codes).view(np.int64).reshape(-1)).cuda()
    dn = torch.full((a.reads,), READ, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    prm = rfx.map_params()
    nh = min(a.host_reads, a.reads)
    ctext = b"".join(b"Contig_%d_%d_%d_%d,%s\n" % (len(x), lr[i, 0], lr[i, 1], i, x) for i, x in enumerate(contigs))
    host_reads = (np.frombuffer(b"ACGT", np.uint8)[codes[:nh]].reshape(-1), np.arange(nh + 1, dtype=np.int64) * READ)
    ms = {"map_ends": [], "map_to_text": [], "map_text": []}
    hits = t = None
    n_text, host = 0, b""
    for i in range(a.runs + 1):                                   # (the first is the warm-up)
        got = {}
        hits = rfx.map_ends(c, dl, dr, dw, dn, a.reads, WPR, prm, hits)
        got["map_ends"] = rfx.last_call_ms
        t, n_text, off = rfx.map_to_text(c, dl, dr, dw, dn, WPR, hits, t)
        got["map_to_text"] = rfx.last_call_ms
        host = rfx.map_text(ctext, host_reads, prm)
        got["map_text"] = rfx.last_call_ms
        if i:
            for k, v in got.items():
                ms[k].append(v)
    assert bytes(t[:len(host)].cpu().numpy()) == host, "the host form and the device entry points disagree"
    h = hits.host()
    n, words = c.n, c.words
    kernel_bytes = {"k_mp_check": 24 * n, "k_mp_seeds": 24 * n + 16 * 2 * n + 48 * n, "k_mp_scan": 8 * WPR * a.reads + 4 * a.reads + 20 * hits.n,
                    "k_mp_text_sizes": 28 * hits.n, "k_mp_text_fill": n_text + 8 * hits.n + 8 * WPR * hits.n}
    print(json.dumps({
        "what": "rfx_dev_map_ends + rfx_dev_map_to_text on a packed contig set and the 2-bit read store, HBM to HBM; rfx_map_text host to host on the first host_reads reads",
        "seed": prm.seed, "min_overlap": prm.min_overlap, "max_mismatch": prm.max_mismatch, "contigs": n, "contig_words": words, "table_entries": 4 * n,
        "reads": a.reads, "read_store_bytes": 8 * WPR * a.reads, "host_reads": nh, "hits": hits.n, "hits_per_read": hits.n / max(a.reads, 1),
        "reads_with_a_hit": int(len(np.unique(h["read"]))), "strand_1_share": float(h["strand"].mean()) if hits.n else None, "text_bytes": n_text,
        "host_text_bytes": len(host), **filter_rates(contigs, codes[:a.sample], prm.seed), **{k: stats(v) for k, v in ms.items()},
        "kernel_bytes": {k: int(v) for k, v in kernel_bytes.items()}}), flush=True)
    rfx.close()


if __name__ == "__main__":
    main()
