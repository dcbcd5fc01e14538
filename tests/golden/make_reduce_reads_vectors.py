#!/usr/bin/env python3
"""Golden vectors for the reduction from reads (rfx_dev_reduce_reads / rfx_reduce_reads): the read sets of
tests/reduce_reads_model.py and, per case, the text of every Count_<k>_reduced that the composed string models give
(tests/reduce_reads_model.py `model`: the CPU oracle's counters, mercy_model, ksort_model, reduce_model) and the counter's row count per
k.  Nothing of the library runs here.

Output: tests/golden/reduce_reads_vectors.npz -- `sets`, `reads/<set>` (+ `_off`), `names`, and per case `<case>/klist`,
`<case>/texts` (+ `_off`: one string per k) and `<case>/rows`."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import reduce_reads_model as RR  # noqa: E402


def pack_strings(strs):
    return np.frombuffer("".join(strs).encode(), np.uint8), np.cumsum([0] + [len(s) for s in strs]).astype(np.int64)


def run_case(c):
    name, (rset, klist, kw) = c
    info = {}
    texts = RR.model(RR.READ_SETS[rset](), klist, info=info, **kw)
    return name, texts, info["rows"] or [0] * len(klist)


def main():
    cases = list(RR.cases().items())
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 1
    if jobs > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(jobs) as pool:
            results = pool.map(run_case, cases, chunksize=1)
    else:
        results = [run_case(c) for c in cases]
    sets = sorted({c[1][0] for c in cases})
    out = {"sets": np.array(sets), "names": np.array([c[0] for c in cases])}
    for s in sets:
        out[f"reads/{s}"], out[f"reads/{s}_off"] = pack_strings(RR.READ_SETS[s]())
    for (name, (rset, klist, kw)), (_, texts, rows) in zip(cases, results):
        out[name + "/klist"] = np.array(klist, np.int64)
        out[name + "/texts"], out[name + "/texts_off"] = pack_strings(texts)
        out[name + "/rows"] = np.array(rows, np.int64)
        print(name, rset, klist, kw, "counter rows", rows, "reduced rows", [t.count("\n") for t in texts], flush=True)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "reduce_reads_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
