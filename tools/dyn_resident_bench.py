"""The dynamic-k passes with the records resident in HBM, on the rows of tools/bench_f2f4.py's dyn block (the (k-1)-mer rows of a
random genome's k-mers, both strands): once as text through rfx_dyn_run_text (host text in, host text out), once already packed
through rfx_dev_dyn_run (device arrays in, device arrays out).  Warm-up on the 1,000-row subset; a host clock around calls that
end in a stream synchronise.  Prints one JSON object per form: wall ms, the algorithmic bytes of the packed layout, hbm_frac."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LUT = np.frombuffer(b"ACGT", np.uint8)


def rows_of_genome(genome_len, k, seed):
    """bench_f2f4.dyn_block's rows: every k-mer of both strands once, shuffled -> [n, k] base codes"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, genome_len).astype(np.uint8)
    n1 = genome_len - k + 1
    fw = g[np.arange(n1)[:, None] + np.arange(k)[None, :]]
    km = np.concatenate([fw, 3 - fw[:, ::-1]])
    return km[rng.permutation(len(km))]


def as_text(km):
    """rows "KMER,1|-1|-1\\n" (form 0)"""
    n, k = km.shape
    tail = np.frombuffer(b",1|-1|-1\n", np.uint8)
    out = np.empty((n, k + len(tail)), np.uint8)
    out[:, :k] = LUT[km]
    out[:, k:] = tail
    return out.tobytes()


def as_records(km):
    from reflexiv_amd.api import DynRecords
    n, k = km.shape
    return DynRecords(np.ascontiguousarray(km[:, :k - 1]).reshape(-1), np.arange(n + 1, dtype=np.int64) * (k - 1),
                      np.ascontiguousarray(km[:, k - 1]), np.arange(n + 1, dtype=np.int64), np.ones(n, np.int32),
                      np.full(n, -1, np.int32), np.full(n, -1, np.int32))


def algorithmic_bytes(n, k, trace):
    """bench_f2f4.dyn_block's formula -- a pass reads and writes every row once; the bases of the set are conserved -- for the packed
    layout: 2 bits per base instead of a byte, and per row 32 bytes of key words + 1 of key_len + 4 of ext_len + 8 of ext_off + 12 of
    marker / left / right = 57; extensions are word-aligned, so their bytes are counted as bases / 4 (a lower bound)"""
    rows_seen = n + sum(trace[:-1])
    ext_bases = n                                             # (one base per input row; merges only concatenate them)
    return 2 * (len(trace) * ext_bases // 4 + 57 * rows_seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--P", type=int, default=8)
    ap.add_argument("--start", type=int, default=5)
    ap.add_argument("--end", type=int, default=14)
    ap.add_argument("--form", choices=("both", "text", "dev"), default="both", help="text: rfx_dyn_run_text only (for a kernel trace of that call)")
    a = ap.parse_args()
    import torch
    import reflexiv_amd
    rfx = reflexiv_amd.Reflexiv(0)
    km = rows_of_genome(a.genome, a.k, 7)
    n = len(km)
    args = (a.P, True, 4, a.start, a.end)
    small_text, text = as_text(km[:1000]), as_text(km)
    if a.form == "dev":
        trace = got = None
    else:
        # as text: host text in, host text out
        rfx.dyn_run_text(small_text, 0, *args)                    # warm-up
        t0 = time.perf_counter()
        got, trace = rfx.dyn_run_text(text, 0, *args)
        wall_text, abi_text = (time.perf_counter() - t0) * 1e3, rfx.last_call_ms
        algo = algorithmic_bytes(n, a.k, trace)
        res = {"rows_in": n, "k": a.k, "P": a.P, "passes": len(trace), "rows_after_each_pass": trace, "algorithmic_bytes": algo}
        print(json.dumps(dict(res, form="dyn_run_text", text_bytes_in=len(text), text_bytes_out=len(got), wall_ms=wall_text,
                              inside_the_c_abi_ms=abi_text, hbm_frac=algo / (abi_text * 1e-3) / 1e9 / 8000.0)), flush=True)
        if a.form == "text":
            rfx.close()
            return
    small, full = rfx.dyn_pack(as_records(km[:1000])), rfx.dyn_pack(as_records(km))
    out_small = type(full)(small.n, small.words)
    out_full = type(full)(full.n, full.words)
    # already packed: device arrays in, device arrays out (the call returns after the stream has drained)
    rfx.dyn_run_dev(small, *args, out=out_small)              # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, trace_dev = rfx.dyn_run_dev(full, *args, out=out_full)
    wall_dev, abi_dev = (time.perf_counter() - t0) * 1e3, rfx.last_call_ms
    if trace is not None:
        assert trace_dev == trace, (trace_dev, trace)
        d_text, ln = rfx.dyn_to_text_dev(out)
        assert bytes(d_text[:ln].cpu().numpy()) == got, "the two forms disagree"
    algo = algorithmic_bytes(n, a.k, trace_dev)
    res = {"rows_in": n, "k": a.k, "P": a.P, "passes": len(trace_dev), "rows_after_each_pass": trace_dev, "algorithmic_bytes": algo}
    print(json.dumps(dict(res, form="dyn_run_dev", rows_out=out.n, ext_words_out=out.words, wall_ms=wall_dev, inside_the_c_abi_ms=abi_dev,
                          hbm_frac=algo / (abi_dev * 1e-3) / 1e9 / 8000.0)), flush=True)
    rfx.close()


if __name__ == "__main__":
    main()
