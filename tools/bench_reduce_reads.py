"""dev helper / bench block: reduce from reads in one resident call (rfx_dev_reduce_reads) at the C2 genome
size.  Input: synthetic reads from rfx_dev_synth_genome / rfx_dev_synth_reads (4.64 Mbp, reads of 150 bases, depth 30) as a 2-bit
read store in HBM.  One warm-up, then --runs runs of rfx_dev_reduce_reads over the k list, timed inside the C ABI
(Reflexiv.last_call_ms); the median and the spread.  Then each packed seam against the text seam it replaces, on the sets of this
input, every call timed the same way (median of --runs after one warm-up):
  A  rfx_dev_ksort_from_counts            vs  rfx_dev_ksort_binarize on the rows in HBM (k <= 31: the rows are rfx_dev_mercy_to_text's
                                              `KMER,1`, the only device printer of counter keys; the packed side gets counts of 1 too)
  B  rfx_dev_reduce_union_packed          vs  two rfx_dev_ksort_to_text + rfx_dev_reduce_union
  C  rfx_dev_dyn_from_kmers               vs  rfx_dev_ksort_to_text + rfx_dev_dyn_binarize form 0
--chain: the whole list also through the entry points without the packed seams (count, rfx_dev_ksort_run, rfx_dev_ksort_to_text,
rfx_dev_reduce_run, rfx_dev_dyn_binarize) with the counter's rows printed on the host outside the timed region; use a smaller --genome.
With the algorithmic bytes of the packed side (65 bytes a record of a set, the counter's keys and counts once) as a fraction of 8 TB/s.
Prints one JSON object.  For per-kernel sums run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_reduce_reads.py
--runs 1` (no counters in that run)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksort import stats  # noqa: E402

REC = 65                      # bytes of one record of a packed set without extension words: 32 key, 1 length, 8 offset, 4 x 4 + 8 ext


def median_ms(rfx, runs, call):
    """one warm-up, then `runs` calls; call() -> its result, or (result, ms) where it adds up several entry points itself (else the
    time is last_call_ms of the one it made) -> (stats, the last result)"""
    ms, res = [], None
    for i in range(runs + 1):
        res = call()
        t = rfx.last_call_ms
        if isinstance(res, tuple) and len(res) == 2 and isinstance(res[1], float):
            res, t = res
        if i:
            ms.append(t)
    return stats(ms), res


def kmer_rows(keys, counts, k):
    """the counter's keys and counts (numpy, on the host) as the rows `KMER,count\n` -> (uint8 text, int64 offsets)"""
    import numpy as np
    W = k // 32 + 1
    keys = keys.reshape(-1, W)
    cols = []
    for j in range(W):
        m = min(32, k - 32 * j)
        cols.append((keys[:, j:j + 1] >> (2 * (m - 1 - np.arange(m))).astype(np.uint64)) & np.uint64(3))
    letters = np.frombuffer(b"ACGT", np.uint8)[np.concatenate(cols, axis=1).astype(np.uint8)]
    rows = [bytes(r) + b"," + str(int(c)).encode() + b"\n" for r, c in zip(letters, counts)]
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return np.frombuffer(b"".join(rows), np.uint8), off


def text_chain(rfx, torch, dw, dn, n_reads, wpr, L, klist, P, runs):
    """the same work through the entry points without the packed seams, device text between them: count, [the rows printed on the host
    and uploaded, NOT timed: no device printer of counter rows exists for k > 31], rfx_dev_ksort_run, per pair two rfx_dev_ksort_to_text
    + rfx_dev_reduce_run, then rfx_dev_ksort_to_text of every Count_<k>_reduced + rfx_dev_dyn_binarize form 0 -> (stats of the timed
    sum, its parts, the records out)"""
    import numpy as np
    E, Es = 8, []
    for i, k in enumerate(klist):
        if ((k >= 61 and klist[1] < 81) or k >= 81) if i == 0 else k >= 61:
            E = 6
        Es.append(E)
    totals, parts, n_out = [], {}, 0
    for run in range(runs + 1):
        t = {"count": 0.0, "ksort_run": 0.0, "to_text": 0.0, "reduce_run": 0.0, "dyn_binarize": 0.0}
        prev, finals = None, []
        for i, k in enumerate(klist):
            W = k // 32 + 1
            cap = n_reads * (L - k + 1) // 2 + 1
            dk = torch.empty(cap * W, dtype=torch.int64, device="cuda")
            dc = torch.empty(cap, dtype=torch.int32 if k <= 31 else torch.int64, device="cuda")
            torch.cuda.synchronize()
            fn = rfx.count_reads_ragged_dev if k <= 31 else rfx.count_reads_ragged_w_dev
            import time
            t0 = time.perf_counter()
            m, _, _ = fn(dw.data_ptr(), dn.data_ptr(), n_reads, wpr, L, k, dk.data_ptr(), dc.data_ptr(), cap)
            t["count"] += (time.perf_counter() - t0) * 1e3
            text, off = kmer_rows(dk[:m * W].cpu().numpy().view(np.uint64), dc[:m].cpu().numpy(), k)      # (not timed)
            d_text, d_off = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off).cuda()
            del dk, dc
            torch.cuda.synchronize()
            cur = rfx.ksort_run(d_text, d_off, rfx.ksort_params(k, max_k=klist[-1], min_error_cov=Es[i]))
            t["ksort_run"] += rfx.last_call_ms
            if i == 0:
                prev = cur
                continue
            k1 = klist[i - 1]
            t1, l1, o1, r1 = rfx.ksort_to_text_dev(prev, k1)
            t["to_text"] += rfx.last_call_ms
            t2, l2, o2, r2 = rfx.ksort_to_text_dev(cur, k)
            t["to_text"] += rfx.last_call_ms
            prev = rfx.reduce_run(t1[:l1], o1[:r1 + 1], t2[:l2], o2[:r2 + 1], P, rfx.reduce_params(k1, k, max_k=klist[-1]))
            t["reduce_run"] += rfx.last_call_ms
            finals.append((prev, k1))
        finals.append((prev, klist[-1]))
        texts, offs, base = [], [torch.zeros(1, dtype=torch.int64, device="cuda")], 0
        for pk, k in finals:
            tx, ln, o, r = rfx.ksort_to_text_dev(pk, k)
            t["to_text"] += rfx.last_call_ms
            texts.append(tx[:ln])
            offs.append(o[1:r + 1] + base)
            base += ln
        d_text, d_off = torch.cat(texts), torch.cat(offs)                                                 # (device copies, not timed)
        torch.cuda.synchronize()
        out = rfx.dyn_binarize_dev(d_text, d_off, 0)
        t["dyn_binarize"] += rfx.last_call_ms
        n_out = out.n
        if run:
            totals.append(sum(t.values()))
            parts = t
    return stats(totals), parts, n_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4_640_000)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--klist", default="23,31,41,53,67,81,95")
    ap.add_argument("--P", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--chain", action="store_true", help="also the whole list through the text entry points (rows printed on the host)")
    a = ap.parse_args()
    import torch
    import reflexiv_amd
    rfx = reflexiv_amd.Reflexiv()
    klist = [int(x) for x in a.klist.split(",")]
    L, wpr = 150, 5
    n_reads = a.genome * a.depth // L
    d_genome = torch.empty((a.genome + 31) // 32 + 1, dtype=torch.int64, device="cuda")
    dw = torch.empty(n_reads * wpr, dtype=torch.int64, device="cuda")
    dn = torch.full((n_reads,), L, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rfx.synth_genome_dev(a.seed, a.genome, d_genome.data_ptr())
    rfx.synth_reads_dev(a.seed, d_genome.data_ptr(), a.genome, 0, n_reads, L, wpr, dw.data_ptr())
    prm = rfx.reduce_reads_params(P=a.P)
    out, per_k = rfx.reduce_reads_dev(dw, dn, n_reads, wpr, L, klist, prm)            # (sizes the output set)
    driver, out = median_ms(rfx, a.runs, lambda: rfx.reduce_reads_dev(dw, dn, n_reads, wpr, L, klist, prm, out)[0])
    chain = None
    if a.chain:
        c_ms, c_parts, c_n = text_chain(rfx, torch, dw, dn, n_reads, wpr, L, klist, a.P, a.runs)
        assert c_n == out.n, (c_n, out.n)
        chain = {"timed_sum_ms": c_ms, "parts_of_the_last_run_ms": c_parts, "records_out": c_n,
                 "not_timed": "printing the counter's rows on the host, their upload, the concatenation of the reduced texts"}

    # ---- the seams, on the sets of the first pair -------------------------------------------------------------------------------
    k1, k2 = klist[0], klist[1]
    seams = {}

    def counted(k):
        W = k // 32 + 1
        cap = n_reads * (L - k + 1) // 2 + 1
        dk = torch.empty(cap * W, dtype=torch.int64, device="cuda")
        dc = torch.empty(cap, dtype=torch.int32 if k <= 31 else torch.int64, device="cuda")
        torch.cuda.synchronize()
        fn = rfx.count_reads_ragged_dev if k <= 31 else rfx.count_reads_ragged_w_dev
        m, _, _ = fn(dw.data_ptr(), dn.data_ptr(), n_reads, wpr, L, k, dk.data_ptr(), dc.data_ptr(), cap)
        return dk[:m * W], dc[:m], m
    dk1, dc1, m1 = counted(k1)
    dk2, dc2, m2 = counted(k2)
    if k1 <= 31:
        ones = torch.ones(m1, dtype=torch.int32, device="cuda")
        d_text, ln, d_off = rfx.mercy_to_text(dk1, m1, k1)
        d_text, d_off = d_text[:ln].clone(), d_off[:m1 + 1].clone()
        torch.cuda.synchronize()
        cp = rfx.ksort_params(k1, max_k=klist[-1])
        t_text, b_text = median_ms(rfx, a.runs, lambda: rfx.ksort_binarize(d_text, d_off, cp))
        t_pk, b_pk = median_ms(rfx, a.runs, lambda: rfx.ksort_from_counts(dk1, ones, cp))
        assert b_text.n == b_pk.n == 2 * m1
        nbytes = m1 * 12 + REC * b_pk.n + 8 * b_pk.n
        seams["A ksort_from_counts"] = {"k": k1, "rows": m1, "text_bytes": int(ln), "text_ms": t_text, "packed_ms": t_pk,
                                        "packed_algorithmic_bytes": int(nbytes), "packed_frac_of_8TBps": nbytes / t_pk["median_ms"] / 1e6 / 8000.0}
    s1 = rfx.ksort_run_counts(dk1, dc1, rfx.ksort_params(k1, max_k=klist[-1]))
    s2 = rfx.ksort_run_counts(dk2, dc2, rfx.ksort_params(k2, max_k=klist[-1]))
    rp = rfx.reduce_params(k1, k2, max_k=klist[-1])

    def union_text():
        t1, l1, o1, r1 = rfx.ksort_to_text_dev(s1, k1)
        ms = rfx.last_call_ms
        t2, l2, o2, r2 = rfx.ksort_to_text_dev(s2, k2)
        ms += rfx.last_call_ms
        u = rfx.reduce_union(t1[:l1], o1[:r1 + 1], t2[:l2], o2[:r2 + 1], rp)
        return (u, l1 + l2), float(ms + rfx.last_call_ms)
    t_text, (u_text, text_bytes) = median_ms(rfx, a.runs, union_text)
    t_pk, u_pk = median_ms(rfx, a.runs, lambda: rfx.reduce_union_packed(s1, s2, rp))
    assert u_text.n == u_pk.n == s1.n + s2.n
    nbytes = 2 * REC * u_pk.n
    seams["B reduce_union_packed"] = {"k1": k1, "k2": k2, "records": u_pk.n, "text_bytes": int(text_bytes), "text_ms": t_text, "packed_ms": t_pk,
                                      "packed_algorithmic_bytes": int(nbytes), "packed_frac_of_8TBps": nbytes / t_pk["median_ms"] / 1e6 / 8000.0}
    f = rfx.reduce_run_packed(s1, s2, a.P, rp)

    def handover_text():
        t, ln, o, r = rfx.ksort_to_text_dev(f, k2)
        ms = rfx.last_call_ms
        d = rfx.dyn_binarize_dev(t[:ln], o[:r + 1], 0)
        return (d, ln), float(ms + rfx.last_call_ms)
    t_text, (h_text, text_bytes) = median_ms(rfx, a.runs, handover_text)
    t_pk, h_pk = median_ms(rfx, a.runs, lambda: rfx.dyn_from_kmers([f], [k2]))
    assert h_text.n == h_pk.n
    nbytes = REC * f.n + (REC + 8) * h_pk.n
    seams["C dyn_from_kmers"] = {"k": k2, "records_in": f.n, "records_out": h_pk.n, "text_bytes": int(text_bytes), "text_ms": t_text, "packed_ms": t_pk,
                                 "packed_algorithmic_bytes": int(nbytes), "packed_frac_of_8TBps": nbytes / t_pk["median_ms"] / 1e6 / 8000.0}
    print(json.dumps({
        "what": "rfx_dev_reduce_reads on synthetic reads in HBM (one call: count, sort, reduce pair by pair, the set of the first-four passes), "
                "and each packed seam against the text seam it replaces",
        "genome": a.genome, "depth": a.depth, "read_len": L, "n_reads": n_reads, "klist": klist, "P": a.P,
        "rows_per_k": per_k, "records_out": out.n, "reduce_reads_ms": driver, "text_chain": chain, "seams": seams}), flush=True)
    rfx.close()


if __name__ == "__main__":
    main()
