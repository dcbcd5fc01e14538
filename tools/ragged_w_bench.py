"""Times the k = 33..63 count of config 2's read set (5 Gbp of PE150 from the 4.64 Mbp genome, -cover 30) synthesised on
the device: (a) rfx_dev_count_reads_w, (b) rfx_dev_count_reads_ragged_w on the same reads with every length 150, (c) the same
words with seeded lengths in 100..150 (the bases past a read's length stay in its words: the count must not read them).
Prints one JSON line: per variant the median, min and max over the timed repetitions, and ns per k-mer instance.

    python tools/ragged_w_bench.py [--k 63] [--gbp 5] [--reps 10] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=63)
    ap.add_argument("--gbp", type=float, default=5.0)
    ap.add_argument("--genome", type=int, default=4_640_000)
    ap.add_argument("--cover", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import numpy as np
    import torch
    import reflexiv_amd
    torch.cuda.set_device(0)
    rfx = reflexiv_amd.Reflexiv(0)
    L, k = 150, a.k
    n = int(a.gbp * 1e9) // L
    wpr = (L + 31) // 32
    dg = torch.empty((a.genome + 31) // 32, dtype=torch.int64, device="cuda")
    dw = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rfx.synth_genome_dev(a.seed, a.genome, dg.data_ptr())
    rfx.synth_reads_dev(a.seed, dg.data_ptr(), a.genome, 0, n, L, wpr, dw.data_ptr())
    rfx.sync()
    del dg
    full = torch.full((n,), L, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(a.seed)
    trimmed = torch.from_numpy(rng.integers(100, L + 1, size=n, dtype=np.int32)).cuda()
    cap = 64 << 20
    dk = torch.empty(cap * 2, dtype=torch.int64, device="cuda")
    dc = torch.empty(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    runs = {
        "a_uniform": lambda: rfx.count_reads_w_dev(dw.data_ptr(), n, wpr, L, k, dk.data_ptr(), dc.data_ptr(), cap, a.cover),
        "b_ragged_all_150": lambda: rfx.count_reads_ragged_w_dev(dw.data_ptr(), full.data_ptr(), n, wpr, L, k, dk.data_ptr(),
                                                                 dc.data_ptr(), cap, a.cover),
        "c_ragged_100_150": lambda: rfx.count_reads_ragged_w_dev(dw.data_ptr(), trimmed.data_ptr(), n, wpr, L, k, dk.data_ptr(),
                                                                 dc.data_ptr(), cap, a.cover),
    }
    out = {"k": k, "gbp": a.gbp, "n_reads": n, "cover": a.cover, "reps": a.reps, "warmup": a.warmup}
    # interleaved rounds: a drift of the clock or the card touches every variant alike
    times = {name: [] for name in runs}
    res = {}
    for rep in range(a.warmup + a.reps):
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= a.warmup:
                times[name].append(dt)
            res[name] = r
    for name, ts in times.items():
        ts = sorted(ts)
        m, nd, inst = res[name]
        med = ts[len(ts) // 2]
        out[name] = {"ms_median": round(med, 2), "ms_min": round(ts[0], 2), "ms_max": round(ts[-1], 2), "instances": inst,
                     "distinct": nd, "kept": m, "ns_per_instance": round(med * 1e6 / max(1, inst), 4)}
    assert res["a_uniform"] == res["b_ragged_all_150"], (res["a_uniform"], res["b_ragged_all_150"])
    out["b_over_a"] = round(out["b_ragged_all_150"]["ms_median"] / out["a_uniform"]["ms_median"], 4)
    out["c_over_a_per_instance"] = round(out["c_ragged_100_150"]["ns_per_instance"] / out["a_uniform"]["ns_per_instance"], 4)
    rfx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
