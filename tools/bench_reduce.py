"""dev helper / bench block: the k-mer reduction stage (Count_<k1>_reduced, Count_<k2>_sorted) at the C2
genome size.  Input: the canonical k-mers of a seeded random genome (4.64 Mbp) at k = 31 and k = 41, both through the sorting
stage (rfx_dev_ksort_run + rfx_dev_ksort_to_text), texts and row offsets already in HBM.  One warm-up, then --runs runs of
rfx_dev_reduce_run + the two rfx_dev_ksort_to_text calls, timed inside the C ABI (Reflexiv.last_call_ms); the median and the
spread.  Then the operators one by one on the same sets: the share of the three rfx_dev_dyn_sort calls, each new operator's time and
its algorithmic bytes (65 bytes per record in and out, the texts once).  Prints one JSON object.  For per-kernel sums run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_reduce.py --runs 1` (no counters in that run)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksort import canonical_kmers, counts_text, stats  # noqa: E402


def sorted_text(rfx, torch, genome, k, seed):
    """Count_<k>_sorted of the genome's canonical k-mers -> (d_text, d_row_off, rows, bytes) in HBM"""
    text, off, _ = counts_text(canonical_kmers(genome, k, seed), seed)
    d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    out = rfx.ksort_run(d_text, d_off, rfx.ksort_params(k))
    d_out, ln, d_row, rows = rfx.ksort_to_text_dev(out, k)
    return d_out[:ln].clone(), d_row[:rows + 1].clone(), rows, ln


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4_640_000)
    ap.add_argument("--k1", type=int, default=31)
    ap.add_argument("--k2", type=int, default=41)
    ap.add_argument("--P", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    import torch
    import reflexiv_amd
    rfx = reflexiv_amd.Reflexiv()
    k1, k2, P = a.k1, a.k2, a.P
    ts, os_, ns, bs = sorted_text(rfx, torch, a.genome, k1, a.seed)
    tl, ol, nl, bl = sorted_text(rfx, torch, a.genome, k2, a.seed)
    torch.cuda.empty_cache()
    cp = rfx.reduce_params(k1, k2)
    run_ms, text_ms = [], []
    out = d1 = d2 = None
    for i in range(a.runs + 1):                                # (the first is the warm-up)
        out = rfx.reduce_run(ts, os_, tl, ol, P, cp, out)
        r = rfx.last_call_ms
        d1, l1, _, rows1 = rfx.ksort_to_text_dev(out, k1, d1, want_offsets=False)
        t = rfx.last_call_ms
        d2, l2, _, rows2 = rfx.ksort_to_text_dev(out, k2, d2, want_offsets=False)
        t += rfx.last_call_ms
        if i:
            run_ms.append(r)
            text_ms.append(t)
    ms, n_of = {}, {}

    def timed(name, res):
        ms[name] = rfx.last_call_ms
        d = res[0] if isinstance(res, tuple) else res
        n_of[name] = d.n
        return res
    u = timed("union", rfx.reduce_union(ts, os_, tl, ol, cp))
    lp = timed("left_prepare", rfx.reduce_left_prepare(u, cp))
    s1, p1 = timed("dyn_sort 1", rfx.dyn_sort_dev(lp, P))
    a1, _ = timed("adjust 0", rfx.reduce_adjust(s1, False, p1, cp))
    rp = timed("right_prepare", rfx.reduce_right_prepare(a1, cp))
    s2, p2 = timed("dyn_sort 2", rfx.dyn_sort_dev(rp, P))
    a2, _ = timed("adjust 1", rfx.reduce_adjust(s2, True, p2, cp))
    fk = timed("full_kmers", rfx.reduce_full_kmers(a2, cp))
    s3, p3 = timed("dyn_sort 3", rfx.dyn_sort_dev(fk, P))
    nt, _ = timed("neutralize", rfx.reduce_neutralize(s3, p3, cp))
    assert nt.n == out.n == rows1 + rows2
    rec = 65
    new_bytes = {"union": bs + bl + rec * u.n, "left_prepare": rec * (u.n + lp.n), "adjust 0": rec * (s1.n + a1.n), "right_prepare": rec * (a1.n + rp.n),
                 "adjust 1": rec * (s2.n + a2.n), "full_kmers": rec * (a2.n + fk.n), "neutralize": rec * (s3.n + nt.n)}
    sorts = ms["dyn_sort 1"] + ms["dyn_sort 2"] + ms["dyn_sort 3"]
    total = [x + y for x, y in zip(run_ms, text_ms)]
    print(json.dumps({
        "what": "rfx_dev_reduce_run + two rfx_dev_ksort_to_text on Count_<k1>_sorted and Count_<k2>_sorted of a random genome, texts in HBM to texts in HBM",
        "k1": k1, "k2": k2, "P": P, "rows_short": ns, "rows_long": nl, "text_in_bytes": int(bs + bl), "records": n_of,
        "rows_out_short": rows1, "rows_out_long": rows2, "text_out_bytes": int(l1 + l2),
        "run_plus_to_text": stats(total), "run": stats(run_ms), "to_text_twice": stats(text_ms),
        "operators_one_by_one_ms": ms, "share_of_the_three_dyn_sort_calls": sorts / sum(ms.values()),
        "new_operators": {n: {"ms_with_its_copies_and_waits": ms[n], "algorithmic_bytes": int(b), "frac_of_8TBps": b / ms[n] / 1e6 / 8000.0}
                          for n, b in new_bytes.items()}}), flush=True)
    rfx.close()


if __name__ == "__main__":
    main()
