"""dev helper / bench block: the mercy k-mer stage (Count_<k>_mercy).  Input: --reads (2,000,000) reads of 150
bases from rfx_dev_synth_reads on a genome of --genome (50,000,000) bases -- depth 6, where the counter with min_cov 2 leaves holes --
and as the solid set what the project's own counter (rfx_dev_count_reads, min_cov 2, k = 31) returns for those reads.  One warm-up, then
--runs runs of rfx_dev_mercy_kmers and rfx_dev_mercy_to_text, each timed inside the C ABI (Reflexiv.last_call_ms), of the host form
rfx_mercy_text on the first --host-reads (50,000) reads with the counter's rows for their windows as text (its uploads, its sort and its copy back
included), and -- for scale only -- of the count stage on the same reads in the same process.  It also MEASURES, on the host: the hits
per window and the mercy k-mers per read of the first --sample (20,000) reads, and the directory's mean and longest bucket.  Prints one
JSON object; "kernel_bytes" in it gives the algorithmic bytes of ONE launch of each kernel (the scan: the read store once, a key and two
offsets per window).  For the per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_mercy.py --runs 1`
(no counters in that run), then `python tools/bench_mercy.py --join STATS RESULT.json`."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksort import stats  # noqa: E402
from bench_fixing import join  # noqa: E402

READ, WPR, K = 150, 5, 31
DIR_BITS = 26                                                      # MC_DIR_BITS of rfx_mercy.hip


def dir_bits(n):
    b = 1
    while b < min(2 * K, DIR_BITS) and (1 << b) < n:
        b += 1
    return b


def windows_of(words):
    """packed reads uint64 [n, 5] -> the canonical k-mers of their windows, uint64 [n, 120]"""
    n = len(words)
    codes = ((words[:, :, None] >> (np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64))) & np.uint64(3)).reshape(n, -1)[:, :READ]
    fw = np.zeros((n, READ - K + 1), np.uint64)
    rc = np.zeros((n, READ - K + 1), np.uint64)
    win = np.lib.stride_tricks.sliding_window_view(codes, K, axis=1)
    for j in range(K):
        fw = (fw << np.uint64(2)) | win[:, :, j]
        rc = (rc << np.uint64(2)) | (np.uint64(3) - win[:, :, K - 1 - j])
    return np.minimum(fw, rc)


def rows_text(keys):
    """keys -> the rows "KMER,2\\n" of a counts file, in pieces"""
    out = []
    sh = np.uint64(2) * np.arange(K - 1, -1, -1, dtype=np.uint64)
    for b in range(0, len(keys), 500000):
        part = keys[b:b + 500000]
        letters = np.frombuffer(b"ACGT", np.uint8)[((part[:, None] >> sh) & np.uint64(3)).astype(np.uint8)]
        out.append(np.concatenate([letters, np.broadcast_to(np.frombuffer(b",2\n", np.uint8), (len(part), 3))], axis=1).tobytes())
    return b"".join(out)


def reads_text(words):
    """packed reads uint64 [n, 5] -> their letters, uint8 [n * 150]"""
    codes = ((words[:, :, None] >> (np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64))) & np.uint64(3)).astype(np.uint8)
    return np.frombuffer(b"ACGT", np.uint8)[codes.reshape(len(words), -1)[:, :READ]].reshape(-1)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--join":
        return join(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--genome", type=int, default=50000000)
    ap.add_argument("--host-reads", type=int, default=50000)
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=28)
    a = ap.parse_args()
    import torch
    import reflexiv_amd
    rfx = reflexiv_amd.Reflexiv()
    n = a.reads
    d_genome = torch.empty((a.genome + 31) // 32, dtype=torch.int64, device="cuda")
    dw = torch.empty(n * WPR, dtype=torch.int64, device="cuda")
    dn = torch.full((n,), READ, dtype=torch.int32, device="cuda")
    cap = n * (READ - K + 1) // 2 + 1
    dk = torch.empty(cap, dtype=torch.int64, device="cuda")
    dc = torch.empty(cap, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rfx.synth_genome_dev(a.seed, a.genome, d_genome.data_ptr())
    rfx.synth_reads_dev(a.seed, d_genome.data_ptr(), a.genome, 0, n, READ, WPR, dw.data_ptr())
    rfx.sync()
    import time
    ms = {"mercy_kmers": [], "mercy_to_text": [], "mercy_text": [], "count_reads_for_scale": []}
    nh = min(a.host_reads, n)
    out = t = rows = host_reads = None
    n_solid = n_text = 0
    host = b""
    for i in range(a.runs + 1):                                   # (the first is the warm-up)
        got = {}
        t0 = time.perf_counter()
        n_solid, distinct, inst = rfx.count_reads_dev(dw.data_ptr(), n, WPR, READ, K, dk.data_ptr(), dc.data_ptr(), cap, 2)
        got["count_reads_for_scale"] = (time.perf_counter() - t0) * 1e3
        out = rfx.mercy_kmers(dk, n_solid, dw, dn, n, WPR, K, out=out)
        got["mercy_kmers"] = rfx.last_call_ms
        t, n_text, _ = rfx.mercy_to_text(out.keys, out.n, K, t, want_offsets=False)
        got["mercy_to_text"] = rfx.last_call_ms
        if i <= 1 and nh > 0:                                     # (the host form once warm and once timed)
            if i == 0:
                words = dw[:nh * WPR].cpu().numpy().view(np.uint64).reshape(nh, WPR)
                keys = np.sort(dk[:n_solid].cpu().numpy().view(np.uint64))
                seen = np.unique(np.concatenate([np.unique(windows_of(words[b:b + 10000])) for b in range(0, nh, 10000)]))
                rows = rows_text(seen[np.isin(seen, keys)][::-1])          # the solid keys these reads can meet, in no useful order
                host_reads = (reads_text(words), np.arange(nh + 1, dtype=np.int64) * READ)
            host = rfx.mercy_text(rows, host_reads, K)
            got["mercy_text"] = rfx.last_call_ms
        if i:
            for k, v in got.items():
                ms[k].append(v)
    assert bytes(t[:len(host)].cpu().numpy()) == host, "the host form and the device entry points disagree"
    # measured on the host: hits per window, mercy k-mers per read, the directory's buckets
    keys = np.sort(dk[:n_solid].cpu().numpy().view(np.uint64))
    ns = min(a.sample, n)
    win = windows_of(dw[:ns * WPR].cpu().numpy().view(np.uint64).reshape(ns, WPR))
    at = np.searchsorted(keys, win.reshape(-1))
    hit = (keys[np.minimum(at, len(keys) - 1)] == win.reshape(-1)).reshape(win.shape) if len(keys) else np.zeros(win.shape, bool)
    b = dir_bits(n_solid)
    buckets = np.bincount((keys >> np.uint64(2 * K - b)).astype(np.int64), minlength=1 << b) if len(keys) else np.zeros(1, np.int64)
    windows = n * (READ - K + 1)
    kernel_bytes = {"k_mc_check": 8 * n_solid, "k_mc_dir": 8 * n_solid + 4 * ((1 << b) + 1),
                    "k_mc_scan": 8 * WPR * n + 4 * n + (8 + 8) * windows + 4 * n + 8 * out.n,      # (both passes share the name: per launch, the count pass)
                    "k_mc_text": 8 * out.n + n_text}
    print(json.dumps({
        "what": "rfx_dev_mercy_kmers + rfx_dev_mercy_to_text on the counter's keys and the 2-bit read store, HBM to HBM; rfx_mercy_text host to host on the first host_reads reads",
        "k": K, "reads": n, "genome": a.genome, "depth": n * READ / a.genome, "read_store_bytes": 8 * WPR * n, "windows": windows, "solid_keys": int(n_solid),
        "mercy_kmers": int(out.n), "mercy_kmers_per_read": out.n / max(n, 1), "text_bytes": int(n_text), "host_reads": nh, "host_text_bytes": len(host),
        "sample_reads": ns, "hits_per_window": float(hit.mean()), "reads_with_every_window_solid": float(hit.all(axis=1).mean()),
        "directory_bits": b, "bucket_mean": float(n_solid / (1 << b)), "bucket_mean_of_used": float(buckets[buckets > 0].mean()) if n_solid else 0.0,
        "bucket_longest": int(buckets.max()), **{k: stats(v) for k, v in ms.items() if v}, "kernel_bytes": {k: int(v) for k, v in kernel_bytes.items()}}), flush=True)
    rfx.close()


if __name__ == "__main__":
    main()
