"""dev helper / bench block: the k-mer sorting stage (Count_<k>_sorted) at the C2 genome size.
Input: a synthetic counts text -- the canonical k-mers of a seeded random genome (4.64 Mbp), one `KMER,NN` row each, counts
10..40 -- already in HBM.  One warm-up, then --runs runs of rfx_dev_ksort_run + rfx_dev_ksort_to_text, timed inside the C ABI
(Reflexiv.last_call_ms); the median and the spread.  The two rfx_dev_dyn_sort calls are timed on their own on the same sets
(their share), and --fixed adds the fixed-k path's chain on the same k-mers at k = 31 (rfx_dev_rc_expand_subkmer, sort, fork
filter, reflect, sort, fork filter) for scale.  Prints one JSON object per k.  For per-kernel sums run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_ksort.py --k 31 --runs 1` (no counters in that run)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LUT = np.frombuffer(b"ACGT", np.uint8)


def canonical_kmers(genome_len, k, seed, chunk=1 << 19):
    """-> uint8 codes [n, k]: the smaller of every k-mer and its reverse complement, in genome order"""
    g = np.random.default_rng(seed).integers(0, 4, genome_len).astype(np.uint8)
    out = []
    for a in range(0, genome_len - k + 1, chunk):
        b = min(a + chunk, genome_len - k + 1)
        fw = np.lib.stride_tricks.sliding_window_view(g[a:b + k - 1], k)
        rv = 3 - fw[:, ::-1]
        d = fw != rv
        j = d.argmax(axis=1)
        r = np.arange(len(fw))
        take_rv = d.any(axis=1) & (rv[r, j] < fw[r, j])
        out.append(np.where(take_rv[:, None], rv, fw))
    return np.concatenate(out)


def counts_text(km, seed):
    """rows `KMER,NN\\n` (fixed width k + 4) -> (uint8 text, int64 row offsets, int32 counts)"""
    n, k = km.shape
    cnt = np.random.default_rng(seed + 1).integers(10, 41, n).astype(np.int32)
    t = np.empty((n, k + 4), np.uint8)
    t[:, :k] = LUT[km]
    t[:, k] = ord(",")
    t[:, k + 1] = ord("0") + cnt // 10
    t[:, k + 2] = ord("0") + cnt % 10
    t[:, k + 3] = ord("\n")
    return t.reshape(-1), np.arange(n + 1, dtype=np.int64) * (k + 4), cnt


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "runs": len(ms)}


def ksort_block(rfx, torch, km, k, seed, runs):
    text, off, _ = counts_text(km, seed)
    d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    n = len(off) - 1
    cp = rfx.ksort_params(k)
    run_ms, text_ms = [], []
    out = d_out = None
    for i in range(runs + 1):                                  # (the first is the warm-up)
        out = rfx.ksort_run(d_text, d_off, cp, out)
        a = rfx.last_call_ms
        d_out, ln, _, rows = rfx.ksort_to_text_dev(out, k, d_out, want_offsets=False)
        if i:
            run_ms.append(a)
            text_ms.append(rfx.last_call_ms)
    # the operators one by one: the share of the two sorts
    s4 = rfx.ksort_binarize(d_text, d_off, cp)
    t_bin = rfx.last_call_ms
    s5, _ = rfx.dyn_sort_dev(s4, 1)
    t_sort1 = rfx.last_call_ms
    f5 = rfx.ksort_fork_filter(s5, False, cp)
    t_fold1 = rfx.last_call_ms
    s6 = rfx.ksort_reflect(f5)
    t_refl = rfx.last_call_ms
    s7, _ = rfx.dyn_sort_dev(s6, 1)
    t_sort2 = rfx.last_call_ms
    f7 = rfx.ksort_fork_filter(s7, True, cp)
    t_fold2 = rfx.last_call_ms
    s8 = rfx.ksort_full_kmers(f7)
    t_full = rfx.last_call_ms
    assert s8.n == out.n == rows
    # algorithmic bytes of the new kernels: the text read once, each record's bytes (32 key + 1 length + 8 extension + 8 offset +
    # 4 extension length + 12 attributes = 65) read and written once per operator, the text written once
    rec = 65
    new_bytes = (len(text) + rec * s4.n) + rec * (s5.n + f5.n) + rec * (f5.n + s6.n) + rec * (s7.n + f7.n) + rec * (f7.n + s8.n) + (rec * s8.n + ln)
    new_ms = t_bin + t_fold1 + t_refl + t_fold2 + t_full + stats(text_ms)["median_ms"]
    total = [a + b for a, b in zip(run_ms, text_ms)]
    return {"what": "rfx_dev_ksort_run + rfx_dev_ksort_to_text on the canonical k-mers of a random genome, text in HBM to text in HBM",
            "k": k, "rows_in": n, "text_in_bytes": int(len(text)), "records_after_step4": s4.n, "after_forward_fold": f5.n,
            "after_reflected_fold": f7.n, "rows_out": rows, "text_out_bytes": ln,
            "run_plus_to_text": stats(total), "run": stats(run_ms), "to_text": stats(text_ms),
            "operators_one_by_one_ms": {"binarize": t_bin, "dyn_sort 1": t_sort1, "fork_filter 0": t_fold1, "reflect": t_refl,
                                        "dyn_sort 2": t_sort2, "fork_filter 1": t_fold2, "full_kmers": t_full},
            "share_of_the_two_dyn_sort_calls": (t_sort1 + t_sort2) / (t_bin + t_sort1 + t_fold1 + t_refl + t_sort2 + t_fold2 + t_full),
            "new_kernels_algorithmic_bytes": int(new_bytes), "new_kernels_ms_with_their_copies_and_waits": new_ms,
            "new_kernels_GBps": new_bytes / new_ms / 1e6, "new_kernels_frac_of_8TBps": new_bytes / new_ms / 1e6 / 8000.0}


def fixed_block(rfx, torch, km, seed):
    """the fixed-k path's chain on the same k-mers at k = 31 (P = 1), each call timed inside the C ABI"""
    import time
    from reflexiv_amd import _lib
    n, k = km.shape
    assert k == 31
    keys = (km.astype(np.uint64) << (np.uint64(2) * np.arange(k - 1, -1, -1, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    cnt = np.random.default_rng(seed + 1).integers(10, 41, n).astype(np.int32)
    o = np.argsort(keys, kind="stable")                        # (the counter hands its k-mers over in ascending order)
    dk, dc = torch.from_numpy(keys[o].view(np.int64)).cuda(), torch.from_numpy(cnt[o]).cuda()

    def recs(cap):
        t = {"key": torch.empty(cap, dtype=torch.int64, device="cuda"), "marker": torch.empty(cap, dtype=torch.int32, device="cuda"),
             "ext_off": torch.empty(cap + 1, dtype=torch.int64, device="cuda"), "ext": torch.empty(cap, dtype=torch.int64, device="cuda"),
             "left": torch.empty(cap, dtype=torch.int32, device="cuda"), "right": torch.empty(cap, dtype=torch.int32, device="cuda")}
        c = _lib.CRecords()
        for f, v in t.items():
            setattr(c, f, v.data_ptr())
        c.cap_n = c.cap_words = cap
        c.key_words = 1
        return t, c
    ps = torch.empty(2, dtype=torch.int64, device="cuda")
    ps2 = torch.empty(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L, ctx = rfx.L, rfx.ctx
    ms = {}

    def timed(name, fn, *a):
        t0 = time.perf_counter()
        st = fn(ctx, *a)
        ms[name] = (time.perf_counter() - t0) * 1e3
        assert st == 0, (name, st, rfx.L.rfx_last_error(ctx))
    for rnd in range(2):                                       # (the first round is the warm-up)
        (ta, a), (tb, b) = recs(2 * n), recs(2 * n)
        p, i64 = C.c_void_p, C.c_int64
        timed("rc_expand_subkmer", L.rfx_dev_rc_expand_subkmer, p(dk.data_ptr()), p(dc.data_ptr()), i64(n), k, C.byref(a))
        a.need_words = a.n
        timed("sort_records 1", L.rfx_dev_sort_records, C.byref(a), 1, k, C.byref(b), p(ps.data_ptr()))
        b.need_words = b.n
        timed("fork_filter 0", L.rfx_dev_fork_filter, 0, C.byref(b), p(ps.data_ptr()), 1, k, 8, 0, C.byref(a), p(ps2.data_ptr()))
        a.need_words = a.n
        timed("reflect_from_forward", L.rfx_dev_reflect_from_forward, C.byref(a), k, C.byref(b))
        b.need_words = b.n
        timed("sort_records 2", L.rfx_dev_sort_records, C.byref(b), 1, k, C.byref(a), p(ps.data_ptr()))
        a.need_words = a.n
        timed("fork_filter 1", L.rfx_dev_fork_filter, 1, C.byref(a), p(ps.data_ptr()), 1, k, 8, 0, C.byref(b), p(ps2.data_ptr()))
        n_out = int(b.n)
    return {"what": "for scale: the fixed-k path's chain on the same k-mers (one-word keys, k = 31), k-mers and counts in HBM, no text",
            "k": k, "kmers_in": n, "records_out": n_out, "calls_ms": ms, "chain_ms": sum(ms.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4_640_000)
    ap.add_argument("--k", type=int, nargs="+", default=[31, 95])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--fixed", action="store_true", help="the fixed-k chain at k = 31 as well")
    a = ap.parse_args()
    import torch
    import reflexiv_amd
    rfx = reflexiv_amd.Reflexiv()
    for k in a.k:
        km = canonical_kmers(a.genome, k, a.seed)
        print(json.dumps(ksort_block(rfx, torch, km, k, a.seed, a.runs)), flush=True)
        if a.fixed and k == 31:
            print(json.dumps(fixed_block(rfx, torch, km, a.seed)), flush=True)
        del km
        torch.cuda.empty_cache()
    rfx.close()


if __name__ == "__main__":
    main()
