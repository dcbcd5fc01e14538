"""dev helper / bench block: the contig fixing stage (Assembly_intermediate/04Fixing).  Input: --contigs
contigs (default 20,000) cut from a seeded random genome so that neighbours overlap by 31 .. 2 (max_k - 30) + 58 bases (their end
chains meet and the loop merges them); lengths 2 max_k + a geometric tail of mean --mean-len (default 1,500) capped at 20,000 bases
-- most contigs short, a few very long, as an assembler's are; both markers, keys of 30 .. max_k - 1 bases; the text and its row
offsets already in HBM.  One warm-up, then --runs runs of rfx_dev_fix_run + rfx_dev_dyn_to_text, timed inside the C ABI
(Reflexiv.last_call_ms); the median and the spread.  Then the operators one by one on the same sets: each new operator's time and
its algorithmic bytes (what it must read and write once: 65 bytes per record + 8 per extension word, in and out; the text once),
the share of the up to 19 rfx_dev_dyn_sort calls and of the loop passes.  Prints one JSON object; "kernel_bytes" in it gives the
algorithmic bytes of ONE launch of every k_fx_* kernel on these sets.  For the per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_fixing.py --runs 1` (no counters in that run: it covers the warm-up, one
run and the operators one by one, so three launches of most kernels), then `python tools/bench_fixing.py --join STATS RESULT.json`
(STATS: the run's kernel_stats CSV or its results .db) prints, per kernel of the stage and per k_dyn_* / sort kernel, the calls, the ms a launch and, for the k_fx_* kernels,
the bytes as a fraction of 8 TB/s."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksort import stats  # noqa: E402


def contig_text(n, mk, mean_len, seed):
    """-> (text bytes as uint8, row offsets, total bases, the longest contig)"""
    rng = np.random.default_rng(seed)
    lens = 2 * mk + np.minimum(rng.geometric(1.0 / mean_len, n), 20000)
    over = rng.integers(31, 2 * (mk - 30) + 59, n)
    starts = np.concatenate([[0], np.cumsum(lens[:-1] - over[:-1])])
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(starts[-1] + lens[-1]))]
    parts, off = [], [0]
    for i in range(n):
        c = g[starts[i]:starts[i] + lens[i]].tobytes()
        m = 1 + int(rng.integers(0, 2))
        kl = int(rng.integers(30, mk)) if mk > 30 else 30
        key, ext = (c[:kl], c[kl:]) if m == 1 else (c[len(c) - kl:], c[:len(c) - kl])
        row = key + b",%d|%d|%d," % (m, int(rng.integers(-40, 41)), int(rng.integers(-40, 41))) + ext + b"\n"
        parts.append(row)
        off.append(off[-1] + len(row))
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(off, np.int64), int(lens.sum()), int(lens.max())


def join(stats, result_json):
    """the kernels of a kernel-trace run (the --stats CSV, or the run's results .db) x the kernel_bytes of a result -> one row per
    kernel, templates of one kernel summed"""
    import re
    res = json.loads([ln for ln in open(result_json) if ln.startswith("{")][-1])
    if stats.endswith(".db"):
        import sqlite3
        rows = sqlite3.connect(stats).execute("select name, count(*), sum(end - start) from kernels group by name").fetchall()
    else:
        import csv
        col = lambda r, *names: next(r[c] for c in r if any(x in c.lower() for x in names))     # noqa: E731
        rows = [(col(r, "name"), int(float(col(r, "calls"))), float(col(r, "totalduration", "total"))) for r in csv.DictReader(open(stats))]
    agg = {}
    for name, calls, ns in rows:
        m = re.search(r"([A-Za-z_]\w*)\s*(<.*>)?\s*\(", name.replace("(anonymous namespace)::", ""))
        a = agg.setdefault(m.group(1) if m else name, [0, 0.0])
        a[0] += calls
        a[1] += ns
    all_ns = sum(a[1] for a in agg.values())
    for short, (calls, ns) in sorted(agg.items(), key=lambda x: -x[1][1]):
        ms = ns / 1e6 / max(calls, 1)
        b = res["kernel_bytes"].get(short)
        print(json.dumps({"kernel": short, "calls": calls, "total_ms": ns / 1e6, "ms_a_launch": ms, "share_of_kernel_time": ns / all_ns,
                          "algorithmic_bytes": b, "frac_of_8TBps": (b / ms / 1e6 / 8000.0) if b and ms > 0 else None}))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--join":
        return join(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=20000)
    ap.add_argument("--mean-len", type=int, default=1500)
    ap.add_argument("--max-k", type=int, default=95)
    ap.add_argument("--P", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=19)
    a = ap.parse_args()
    import torch
    import reflexiv_amd
    rfx = reflexiv_amd.Reflexiv()
    mk, P = a.max_k, a.P
    text, off, bases, longest = contig_text(a.contigs, mk, a.mean_len, a.seed)
    d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    cp = rfx.fix_params(mk)
    run_ms, text_ms = [], []
    out = d_out = None
    for i in range(a.runs + 1):                                # (the first is the warm-up)
        out = rfx.fix_run(d_text, d_off, P, cp, out)
        r = rfx.last_call_ms
        d_out, ln = rfx.dyn_to_text_dev(out, d_out)
        if i:
            run_ms.append(r)
            text_ms.append(rfx.last_call_ms)
    ms, n_of, w_of = {}, {}, {}

    def timed(name, res):
        ms[name] = rfx.last_call_ms
        d = res[0] if isinstance(res, tuple) else res
        n_of[name], w_of[name] = d.n, d.words
        return res
    b = timed("binarize", rfx.fix_binarize(d_text, d_off, cp))
    lg, d_k, nk = timed("contig_ends", rfx.fix_contig_ends(b, cp))
    u = timed("kmer_set", rfx.fix_kmer_set(d_k, nk, lg))
    s1, p1 = timed("dyn_sort 1", rfx.dyn_sort_dev(u, P))
    f1, _ = timed("fork_filter 0", rfx.fix_fork_filter(s1, False, p1))
    rf = timed("reflect", rfx.fix_reflect(f1))
    s2, p2 = timed("dyn_sort 2", rfx.dyn_sort_dev(rf, P))
    f2, o2 = timed("fork_filter 1", rfx.fix_fork_filter(s2, True, p2))
    cur, _ = timed("loop pass 0", rfx.dyn_extend_pass_dev(f2, o2, stage=1, start_iteration=5, start_marker=2))
    trace = [cur.n]
    for i in range(1, 18):
        s, ps = timed(f"dyn_sort {i + 2}", rfx.dyn_sort_dev(cur, P))
        cur, _ = timed(f"loop pass {i}", rfx.dyn_extend_pass_dev(s, ps, stage=1, start_iteration=5, start_marker=2))
        trace.append(cur.n)
    assert cur.n == out.n
    size = lambda name: 65 * n_of[name] + 8 * w_of[name]        # noqa: E731
    new_bytes = {"binarize": len(text) + size("binarize"), "contig_ends": size("binarize") + size("contig_ends") + 8 * nk,
                 "kmer_set": 8 * nk + size("contig_ends") + size("kmer_set"), "fork_filter 0": size("dyn_sort 1") + size("fork_filter 0"),
                 "reflect": size("fork_filter 0") + size("reflect"), "fork_filter 1": size("dyn_sort 2") + size("fork_filter 1")}
    rec, nb = 65, n_of["binarize"]                              # one launch of every kernel of the stage on these sets
    fold = lambda src, dst: {"k_fx_key_heads": 8 * n_of[src] + 4 * n_of[src], "k_fx_fold_contest": (4 + 8 + 4 + 8) * n_of[src],     # noqa: E731
                             "k_fx_fold_keep": (4 + 8 + 4 + 8 + 4) * n_of[src], "k_fx_index": 12 * n_of[src] + 8 * n_of[dst],
                             "k_fx_gather_rec": (8 + rec - 8) * n_of[dst] * 2, "k_fx_gather_ext": 16 * w_of[dst] + 8 * w_of[dst]}
    kernel_bytes = {"k_fx_long_enough": 9 * a.contigs, "k_fx_ends_sizes": 17 * nb, "k_fx_ends_kmers": 8 * nk + 16 * nk,   # (a 31-mer out, two words of its contig in)
                    "k_fx_ends_long": size("binarize") + size("contig_ends"), "k_fx_iota": 4 * nk, "k_fx_value_heads": 12 * nk,
                    "k_fx_set_kmers": 20 * nk + rec * (n_of["kmer_set"] - n_of["contig_ends"]), "k_fx_set_long": 2 * size("contig_ends"),
                    "k_fx_check": 5 * n_of["dyn_sort 1"], "k_fx_reflect": size("fork_filter 0") + size("reflect")}
    kernel_bytes.update(fold("dyn_sort 1", "fork_filter 0"))    # (the second fold's sets are a little smaller)
    sorts = sum(v for k, v in ms.items() if k.startswith("dyn_sort"))
    passes = sum(v for k, v in ms.items() if k.startswith("loop pass"))
    total = [x + y for x, y in zip(run_ms, text_ms)]
    print(json.dumps({
        "what": "rfx_dev_fix_run + rfx_dev_dyn_to_text on the rows of a seeded contig set, text in HBM to text in HBM",
        "max_k": mk, "P": P, "contigs": a.contigs, "bases": bases, "longest_contig": longest, "text_in_bytes": int(len(text)),
        "end_31mers": nk, "records": n_of, "records_behind_each_loop_pass": trace, "rows_out": out.n, "text_out_bytes": int(ln),
        "run_plus_to_text": stats(total), "run": stats(run_ms), "to_text": stats(text_ms),
        "operators_one_by_one_ms": ms, "share_of_the_19_dyn_sort_calls": sorts / sum(ms.values()),
        "share_of_the_18_loop_passes": passes / sum(ms.values()),
        "kernel_bytes": {k: int(v) for k, v in kernel_bytes.items()},
        "new_operators": {n: {"ms_with_its_copies_and_waits": ms[n], "algorithmic_bytes": int(v), "frac_of_8TBps": v / ms[n] / 1e6 / 8000.0}
                          for n, v in new_bytes.items()}}), flush=True)
    rfx.close()


if __name__ == "__main__":
    main()
