"""dev helper / bench block: the contig extension stages (08Extend, 09ExtendAgain).  Input: the set that
tools/bench_endext.py's input leaves behind rfx_dev_endext_contigs -- --contigs contigs (10,000; 200 to 1,800 bases) with the consensus
ends of --rows-per-end (30) alignment rows per end, max_k 95 -- resident in HBM.  One warm-up, then --runs runs of rfx_dev_ext_run, of
the three calls of 09 on its resident output (rfx_dev_fix2_run, rfx_dev_fix2_contigs, rfx_dev_ext2_to_text), each timed inside the C ABI
(Reflexiv.last_call_ms), and of the two host forms rfx_ext_text and rfx_ext2_text (their uploads and copies back included); the median
and the spread of each.  The tool asserts that the device chain's texts equal the host forms'.  Prints one JSON object; "kernel_bytes"
in it gives the algorithmic bytes of ONE launch of the new kernels.  For the per-kernel times run it under `rocprofv3 --kernel-trace
--stats -- python tools/bench_extend.py --runs 1` (no counters in that run), then `python tools/bench_extend.py --join STATS
RESULT.json`; --fix-run adds one rfx_dev_fix_run on rows that give as many end 31-mers, for k_fx_ends_kmers beside k_ex_ends_kmers."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksort import stats  # noqa: E402
from bench_fixing import join  # noqa: E402
from bench_endext import synthesize, LETTERS  # noqa: E402


def text_of(t, n):
    return bytes(t[:n].cpu().numpy())


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--join":
        return join(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=10000)
    ap.add_argument("--rows-per-end", type=int, default=30)
    ap.add_argument("--max-k", type=int, default=95)
    ap.add_argument("--partition", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=24)
    ap.add_argument("--fix-run", action="store_true")
    a = ap.parse_args()
    import torch
    import reflexiv_amd
    rfx = reflexiv_amd.Reflexiv()
    contigs, lr, text, off, _ = synthesize(a.contigs, a.rows_per_end, a.seed)
    c = rfx.contigs_pack([x.decode() for x in contigs])
    dl, dr = torch.from_numpy(np.ascontiguousarray(lr[:, 0])).cuda(), torch.from_numpy(np.ascontiguousarray(lr[:, 1])).cuda()
    d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    s = rfx.endext_contigs(c, dl, dr, rfx.endext_consensus(c, dl, dr, d_text, d_off), a.max_k)
    t07, n07 = rfx.endext_to_text(s)
    text07 = text_of(t07, n07)
    prm = rfx.fix_params(a.max_k)
    P = a.partition
    ms = {"ext_run": [], "fix2_run": [], "fix2_contigs": [], "ext2_to_text": [], "ext_text": [], "ext2_text": []}
    out = out2 = cs = t8 = t9 = None
    n8 = n9 = 0
    host8 = host9 = b""
    for i in range(a.runs + 1):                                   # (the first is the warm-up)
        got = {}
        out = rfx.ext_run(s, P, prm, out)
        got["ext_run"] = rfx.last_call_ms
        out2 = rfx.fix2_run(out, P, prm, out2)
        got["fix2_run"] = rfx.last_call_ms
        cs, dl2, dr2 = rfx.fix2_contigs(out2, prm, cs)
        got["fix2_contigs"] = rfx.last_call_ms
        t9, n9 = rfx.ext2_to_text(cs, t9)
        got["ext2_to_text"] = rfx.last_call_ms
        t8, n8 = rfx.dyn_to_text_dev(out, t8)
        host8 = rfx.ext_text(text07, P, prm)
        got["ext_text"] = rfx.last_call_ms
        host9 = rfx.ext2_text(host8, P, prm)
        got["ext2_text"] = rfx.last_call_ms
        if i:
            for k, v in got.items():
                ms[k].append(v)
    assert host8 == text_of(t8, n8), "08Extend: the host form and the device chain disagree"
    assert host9 == text_of(t9, n9), "09ExtendAgain: the host form and the device chain disagree"
    lg, d_k, n31 = rfx.ext_contig_ends(s, prm)
    extra = {}
    if a.fix_run:                                                  # as many end 31-mers from the fixing stage's own contig ends
        rng = np.random.default_rng(a.seed)
        per = 2 * (a.max_k - 30)
        rows = []
        for _ in range(max(1, n31 // per)):
            b = LETTERS[rng.integers(0, 4, 2 * a.max_k + 200)].tobytes().decode()
            rows.append(f"{b[:30]},1|-1|-1,{b[30:]}\n")
        ft = torch.from_numpy(np.frombuffer("".join(rows).encode(), np.uint8).copy()).cuda()
        fo = np.zeros(len(rows) + 1, np.int64)
        fo[1:] = np.cumsum([len(r) for r in rows])
        fo = torch.from_numpy(fo).cuda()
        torch.cuda.synchronize()
        rfx.fix_run(ft, fo, P, rfx.fix_params(a.max_k, max_iteration=-1))
        extra = {"fix_run_rows": len(rows), "fix_run_kmers": len(rows) * per, "fix_run_ms": rfx.last_call_ms}
    n = s.n
    kernel_bytes = {"k_ex_ends_sizes": 36 * n, "k_ex_ends_kmers": 8 * n31 + 8 * s.set.words + 40 * n, "k_ex_ends_long": 8 * s.set.words + 8 * lg.words + 104 * lg.n,
                    "k_fx2_text_fill": 8 * cs.words + 16 * cs.n + n9}
    print(json.dumps({
        "what": "rfx_dev_ext_run on the resident set of rfx_dev_endext_contigs, the calls of 09 on its resident output, HBM to HBM; rfx_ext_text and rfx_ext2_text host to host",
        "max_k": a.max_k, "P": P, "contigs_in": n, "set_words": s.set.words, "flagged": int((s.flags[:n] != 0).sum().item()), "end_kmers": n31, "long_words": lg.words,
        "records_08": out.n, "text_08_bytes": n8, "records_09": out2.n, "contigs_09": cs.n, "text_09_bytes": n9, "text_07_bytes": n07,
        **{k: stats(v) for k, v in ms.items()}, **extra, "kernel_bytes": {k: int(v) for k, v in kernel_bytes.items()}}), flush=True)
    rfx.close()


if __name__ == "__main__":
    main()
