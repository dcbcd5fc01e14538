"""dev helper / bench block: the second contig fixing stage (05FixingAgain, 06ContigEnds).  Input: the packed
output of rfx_dev_fix_run on the contig set of tools/bench_fixing.py (--contigs 20,000, --max-k 95, --P 8, --seed 19), resident in
HBM.  One warm-up, then --runs runs of rfx_dev_fix2_run + rfx_dev_fix2_contigs + rfx_dev_fix2_to_text + rfx_dev_fix2_ends_text, each
timed inside the C ABI (Reflexiv.last_call_ms); the median and the spread of their sum and of each.  Then the two text writers on
the SAME record set, --runs times each: rfx_dev_dyn_to_text (k_dyn_text_fill: one thread and one search per output byte) against
rfx_dev_fix2_to_text (k_fx2_text_fill: one thread, one search and one 16-byte store per 16 output bytes), as ns per output byte.
Prints one JSON object; "kernel_bytes" in it gives the algorithmic bytes of ONE launch of the stage's kernels and of
k_dyn_text_fill on these sets.  For the per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python
tools/bench_fixing2.py --runs 1` (no counters in that run), then `python tools/bench_fixing2.py --join STATS RESULT.json`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksort import stats  # noqa: E402
from bench_fixing import contig_text, join  # noqa: E402


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
    fixed = rfx.fix_run(d_text, d_off, P, cp)                     # the stage's input: a packed set, no text in between
    ms = {"run": [], "contigs": [], "to_text": [], "ends_text": []}
    out = c = dl = dr = t1 = t2 = None
    n1 = n2 = 0
    for i in range(a.runs + 1):                                   # (the first is the warm-up)
        got = {}
        out = rfx.fix2_run(fixed, P, cp, out)
        got["run"] = rfx.last_call_ms
        c, dl, dr = rfx.fix2_contigs(out, cp, c, dl, dr)
        got["contigs"] = rfx.last_call_ms
        t1, n1 = rfx.fix2_to_text(c, dl, dr, t1)
        got["to_text"] = rfx.last_call_ms
        t2, n2 = rfx.fix2_ends_text(c, dl, dr, t2)
        got["ends_text"] = rfx.last_call_ms
        if i:
            for k, v in got.items():
                ms[k].append(v)
    total = [sum(ms[k][i] for k in ms) for i in range(a.runs)]
    # the two writers on the same record set
    old_ms, new_ms, d_old, n_old = [], [], None, 0
    for i in range(a.runs + 1):
        d_old, n_old = rfx.dyn_to_text_dev(out, d_old)
        o = rfx.last_call_ms
        t1, n1 = rfx.fix2_to_text(c, dl, dr, t1)
        if i:
            old_ms.append(o)
            new_ms.append(rfx.last_call_ms)
    words = c.words
    kernel_bytes = {"k_fx2_check": 5 * fixed.n, "k_fx2_cat_sizes": 5 * out.n + 8 * out.n,
                    "k_fx2_cat": 65 * out.n + 8 * out.words + 8 * words + 24 * c.n,
                    "k_fx2_text_sizes": 24 * c.n + 8 * c.n, "k_fx2_text_fill": 8 * words + 24 * c.n + n1,      # (to_text's launch)
                    "k_dyn_text_fill": 65 * out.n + 8 * out.words + n_old}
    print(json.dumps({
        "what": "rfx_dev_fix2_run + _contigs + _to_text + _ends_text on the packed output of rfx_dev_fix_run, HBM to HBM",
        "max_k": mk, "P": P, "contigs_in": a.contigs, "bases_in": bases, "records_in": fixed.n, "records_behind_the_loop": out.n,
        "contigs_out": c.n, "contig_words": words, "text_bytes": n1, "ends_bytes": n2, "rounds": min(int(cp.max_iteration) + 1, 29),
        "all_four": stats(total), **{k: stats(v) for k, v in ms.items()},
        "writers_on_the_same_set": {
            "k_dyn_text_fill": {"bytes": n_old, "ms": stats(old_ms), "ns_per_byte": stats([1e6 * x / max(n_old, 1) for x in old_ms])},
            "k_fx2_text_fill": {"bytes": n1, "ms": stats(new_ms), "ns_per_byte": stats([1e6 * x / max(n1, 1) for x in new_ms])}},
        "kernel_bytes": {k: int(v) for k, v in kernel_bytes.items()}}), flush=True)
    rfx.close()


if __name__ == "__main__":
    main()
