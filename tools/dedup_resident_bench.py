"""The contig de-duplication with the contigs resident in HBM, on the contigs of tools/bench_f2f4.py's dedup block (N random
contigs + their reverse complements, shuffled), three ways: the host form (rfx_dedup_contigs: host strings in, host strings out),
as text through rfx_dedup_contig_text (host text in, host text out), and already packed through rfx_dev_dedup_contigs (device
arrays in, device arrays out).  One warm-up on 64 contigs; a host clock around calls that end in a stream synchronise.  Prints
one JSON object per form: wall ms, ms inside the C ABI, the algorithmic bytes of the packed layout, hbm_frac."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LUT = np.frombuffer(b"ACGT", np.uint8)


def contigs_of(n_pairs, seed=5, lo=600, hi=3000):
    """bench_f2f4.dedup_block's contigs"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi, n_pairs)
    off = np.zeros(n_pairs + 1, np.int64)
    off[1:] = np.cumsum(lens)
    codes = rng.integers(0, 4, int(off[-1])).astype(np.uint8)
    contigs = []
    for i in range(n_pairs):
        c = codes[off[i]:off[i + 1]]
        contigs.append(LUT[c].tobytes().decode())
        contigs.append(LUT[3 - c[::-1]].tobytes().decode())
    return [contigs[i] for i in rng.permutation(len(contigs))]


def as_text(contigs):
    """the contig text the path writes: ">Contig-<len>-<idx>" and the sequence at 100 columns"""
    return "".join(f">Contig-{len(s)}-{i}\n" + "".join(s[j:j + 100] + "\n" for j in range(0, len(s), 100)) for i, s in enumerate(contigs))


def report(form, contigs_in, bases_in, rounds, bases_out, wall, abi, **more):
    """bench_f2f4.dedup_block's formula -- every base read once and every surviving base written once -- at a quarter byte per base"""
    algo = (bases_in + bases_out) // 4
    print(json.dumps(dict(form=form, contigs_in=contigs_in, bases_in=bases_in, contigs_after_each_round=rounds, bases_out=bases_out,
                          wall_ms=wall, inside_the_c_abi_ms=abi, algorithmic_bytes=algo, hbm_frac=algo / (abi * 1e-3) / 1e9 / 8000.0, **more)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000)
    ap.add_argument("--form", choices=("all", "host", "text", "dev"), default="all", help="one form only (for a kernel trace of that call)")
    a = ap.parse_args()
    import torch
    import reflexiv_amd
    rfx = reflexiv_amd.Reflexiv(0)
    contigs = contigs_of(a.pairs)
    small = contigs[:64]
    total = sum(map(len, contigs))
    surv = text_out = None
    if a.form in ("all", "host"):
        rfx.dedup_contigs(small, 500)                             # warm-up
        t0 = time.perf_counter()
        surv, text_out, rounds = rfx.dedup_contigs(contigs, 500)
        wall, abi = (time.perf_counter() - t0) * 1e3, rfx.last_call_ms
        report("dedup_contigs (host strings)", len(contigs), total, rounds, sum(map(len, surv)), wall, abi, contigs_out=len(surv))
    if a.form in ("all", "text"):
        small_text, text = as_text(small), as_text(contigs)
        rfx.dedup_contig_text(small_text, 500)                    # warm-up
        src = text.encode()
        cap = len(src) + 4096
        import ctypes as C
        out = np.empty(cap, np.uint8)
        ln, nc, rn = C.c_int64(0), C.c_int64(0), (C.c_int64 * 3)()
        t0 = time.perf_counter()
        st = rfx.L.rfx_dedup_contig_text(rfx.ctx, src, C.c_int64(len(src)), 500, out.ctypes.data_as(C.c_void_p), C.c_int64(cap), C.byref(ln), C.byref(nc), rn)
        wall = abi = (time.perf_counter() - t0) * 1e3             # (the call itself: the clock is around the C ABI)
        assert st == 0, st
        got = bytes(out[:ln.value]).decode()
        if text_out is not None:
            assert got == text_out, "the text form and the host form disagree"
        bases_out = sum(int(h.split("-")[1]) for h in got.split("\n") if h.startswith(">"))
        report("dedup_contig_text (host text)", len(contigs), total, [int(x) for x in rn], bases_out, wall, abi, text_bytes_in=len(src),
               text_bytes_out=int(ln.value), contigs_out=int(nc.value))
    if a.form in ("all", "dev"):
        pk_small, pk = rfx.contigs_pack(small), rfx.contigs_pack(contigs)
        out_small, out_full = type(pk)(pk_small.n, pk_small.words), type(pk)(pk.n, pk.words)
        rfx.dedup_dev(pk_small, out=out_small)                    # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, rounds = rfx.dedup_dev(pk, out=out_full)
        wall, abi = (time.perf_counter() - t0) * 1e3, rfx.last_call_ms
        assert out is out_full, "the output did not fit the input's sizes"
        got = rfx.contigs_unpack(out)
        if surv is not None:
            assert got == surv, "the packed form and the host form disagree"
        report("dedup_dev (packed, resident)", len(contigs), total, rounds, sum(map(len, got)), wall, abi, contigs_out=out.n, words_out=out.words)
    rfx.close()


if __name__ == "__main__":
    main()
