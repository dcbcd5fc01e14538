"""dev helper / bench block: the end extension of contigs from alignment rows (07EndExtend).  Input: --contigs
contigs (10,000; 200 to 1,800 bases) as a packed set in HBM and --rows-per-end (30) alignment rows per contig end, synthesized as
tests/golden/make_endext_vectors.py synthesizes them -- reads that overhang the end by 1..149 bases behind a start or a tail of 0..12,
one base in 25 replaced by another letter, a lower-case letter or N -- shuffled, as text in HBM.  One warm-up, then --runs runs of
rfx_dev_endext_consensus + rfx_dev_endext_contigs + rfx_dev_endext_to_text, each timed inside the C ABI (Reflexiv.last_call_ms), and of
the host form rfx_endext_text (its upload and copy back included); the median and the spread of each.  Prints one JSON object;
"kernel_bytes" in it gives the algorithmic bytes of ONE launch of the pile-up and of the text fill.  For the per-kernel times run it
under `rocprofv3 --kernel-trace --stats -- python tools/bench_endext.py --runs 1` (no counters in that run), then `python
tools/bench_endext.py --join STATS RESULT.json`."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksort import stats  # noqa: E402
from bench_fixing import join  # noqa: E402

LETTERS = np.frombuffer(b"ACGT", np.uint8)
NOISE = np.frombuffer(b"ACGTacgtNN", np.uint8)


def synthesize(n, per_end, seed):
    """-> (contigs: list of bytes, left / right int32, the row text as a uint8 array, its row offsets, the bases the rows contribute)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(200, 1800, n)
    contigs = [LETTERS[rng.integers(0, 4, int(L))].tobytes() for L in lens]
    lr = rng.integers(-3, 4, (n, 2)).astype(np.int32)
    rows, seq_at, seq_len, contributed = [], [], [], 0
    for i, c in enumerate(contigs):
        L = len(c)
        two = L >= 400
        ident = b"Contig_%d_%d_%d_%d" % (L, lr[i, 0], lr[i, 1], i)
        ext_l, ext_r = LETTERS[rng.integers(0, 4, 340)].tobytes(), LETTERS[rng.integers(0, 4, 340)].tobytes()
        par = rng.integers(0, 1 << 30, (per_end, 6))
        for a in par:
            ref = c[:200] if two else c
            s, start, m = 1 + int(a[0]) % 149, 1 + int(a[1]) % 12, 20 + int(a[2]) % 80
            o = s - start
            clip = ext_l[:o + 1][::-1] + ref[:s - o - 1] if o >= 0 else ref[start - s - 1:start - 1]
            head = ident + (b"-L" if two else b"") + b"\t%d\t%dS%dM\t" % (start, s, m)
            seq = clip + ref[start - 1:start - 1 + m]
            rows.append(head + seq + b"\n")
            seq_at.append(len(head))
            seq_len.append(len(seq))
            contributed += o + 1 if o > 0 and start < 10 else 0
            ref = c[L - 200:] if two else c
            s, tail, m = 1 + int(a[3]) % 149, int(a[4]) % 13, 20 + int(a[5]) % 80
            start = len(ref) - m - tail + 1
            head = ident + (b"-R" if two else b"") + b"\t%d\t%dM%dS\t" % (start, m, s)
            seq = ref[start - 1:start - 1 + m] + (ref[len(ref) - tail:] + ext_r)[:s]
            rows.append(head + seq + b"\n")
            seq_at.append(len(head))
            seq_len.append(len(seq))
            contributed += s - tail if s > tail and tail < 10 else 0
    order = rng.permutation(len(rows))
    rows = [rows[j] for j in order]
    seq_at, seq_len = np.array(seq_at, np.int64)[order], np.array(seq_len, np.int64)[order]
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    text = np.frombuffer(b"".join(rows), np.uint8).copy()
    # noise on the bases only: one in 25
    first = np.repeat(off[:-1] + seq_at, seq_len)
    pos = first + (np.arange(len(first)) - np.repeat(np.cumsum(seq_len) - seq_len, seq_len))
    hit = pos[rng.random(len(pos)) < 0.04]
    text[hit] = NOISE[rng.integers(0, 10, len(hit))]
    return contigs, lr, text, off, contributed


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--join":
        return join(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=10000)
    ap.add_argument("--rows-per-end", type=int, default=30)
    ap.add_argument("--max-k", type=int, default=95)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=24)
    a = ap.parse_args()
    import torch
    import reflexiv_amd
    rfx = reflexiv_amd.Reflexiv()
    contigs, lr, text, off, contributed = synthesize(a.contigs, a.rows_per_end, a.seed)
    c = rfx.contigs_pack([x.decode() for x in contigs])
    dl, dr = torch.from_numpy(np.ascontiguousarray(lr[:, 0])).cuda(), torch.from_numpy(np.ascontiguousarray(lr[:, 1])).cuda()
    d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    ctext = b"".join(b"Contig_%d_%d_%d_%d,%s\n" % (len(x), lr[i, 0], lr[i, 1], i, x) for i, x in enumerate(contigs))
    rtext = text.tobytes()
    ms = {"consensus": [], "contigs": [], "to_text": [], "host_form": []}
    cons = s = t = None
    n_text, host = 0, b""
    for i in range(a.runs + 1):                                   # (the first is the warm-up)
        got = {}
        cons = rfx.endext_consensus(c, dl, dr, d_text, d_off, cons)
        got["consensus"] = rfx.last_call_ms
        s = rfx.endext_contigs(c, dl, dr, cons, a.max_k, s)
        got["contigs"] = rfx.last_call_ms
        t, n_text = rfx.endext_to_text(s, t)
        got["to_text"] = rfx.last_call_ms
        host = rfx.endext_text(ctext, rtext, a.max_k)
        got["host_form"] = rfx.last_call_ms
        if i:
            for k, v in got.items():
                ms[k].append(v)
    assert host == bytes(t[:n_text].cpu().numpy()), "the host form and the device entry points disagree"
    n, rows = c.n, len(off) - 1
    total = [sum(ms[k][i] for k in ("consensus", "contigs", "to_text")) for i in range(a.runs)]
    kernel_bytes = {"k_ee_parse": len(text) + 8 * rows + 44 * rows, "k_ee_pile": 36 * rows + contributed + 16 * n + 172 * n,
                    "k_ee_splice": 8 * (c.words + cons.left.words + cons.right.words) + 8 * s.set.words + 80 * n,
                    "k_ee_text_fill": 8 * s.set.words + 44 * s.n + n_text}
    print(json.dumps({
        "what": "rfx_dev_endext_consensus + _contigs + _to_text on a packed contig set and alignment rows, HBM to HBM; rfx_endext_text host to host",
        "max_k": a.max_k, "contigs_in": n, "contig_words": c.words, "rows": rows, "row_bytes": len(text), "bases_contributed": int(contributed),
        "left_consensus_words": cons.left.words, "right_consensus_words": cons.right.words, "flagged": int((cons.flags[:n] != 0).sum().item()),
        "contigs_out": s.n, "spliced_words": s.set.words, "text_bytes": n_text,
        "all_three": stats(total), **{k: stats(v) for k, v in ms.items()}, "kernel_bytes": {k: int(v) for k, v in kernel_bytes.items()}}), flush=True)
    rfx.close()


if __name__ == "__main__":
    main()
