#!/usr/bin/env python3
"""Edge vectors for the dynamic-k passes made by the REFERENCE'S OWN classes, fed with CRAFTED row sets.

The sibling of make_dynamic_vectors.py and the same route (the reference's operator classes through tools/java2py.py, the
order contract between two classes), but the rows are not k-mers cut from a genome: they are the families of
tests/pymodel.dyn_crafted_families -- keys that are prefixes of one random 94-base string, of the lengths
{22, 30, 31, 32, 40, 61, 62, 63, 80, 92, 93, 94} at which the terminator moves into bit 0 of a block or into a new block,
either marker, left / right from negatives, 0, positives below and above the partner's extension length and +-29990, and
extensions of 1..40 bases (longer than the shortest keys).  The text rows go through Iteration's
DynamicKmerBinarizerFromReducedToSubKmer; then, per pass, sort("k-1"), the cut into P partitions, and

  stage 1: DSExtendReflexivKmerToArrayLoop with param.startIteration 5 or 61, and once with param.scramble == 3 (the
           emission marker starts at 1);
  stage 0: FirstFour's DSExtendReflexivKmer on the same rows with the extension as ONE long.

What the reference classes could not take, and is therefore covered against the oracle only (tests/test_gpu_dynamic_edges.py):
  - stage 0 with an extension of more than 15 bases, or a second stage 0 pass over merged rows: FirstFour keeps the
    extension in one long (31 bases) and a merge joins two extensions, so the crafted stage 0 rows carry 1..15 bases and
    the case records a single pass;
  - keys of 95..124 bases: the classes would take them, but the reference's k-mer list ends at k = 95 (a 94-base key), and
    the vectors stay inside what the reference can produce;
  - a key of 125 bases or more, P = 0 and P > 63: refusals of this library's entry points, which the reference does not have.

Output: tests/golden/dynamic_edge_vectors.npz -- per case `meta` = [P, stage, startIteration, start marker, passes], `in`
(the crafted text rows) and `pass<i>` (the text rows after sort + pass i, each pass fed with the one before)."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import java2py as jp  # noqa: E402
import pymodel  # noqa: E402
from make_reference_vectors import make_param, drain  # noqa: E402
from make_dynamic_vectors import op, run_partitions, to_text, pack_rows  # noqa: E402

# (name, families, P, stage, startIteration, param.scramble, passes, longest extension)
CASES = [("e0", 300, 3, 0, 0, 2, 1, 15), ("e1", 300, 7, 1, 5, 2, 3, 40), ("e2", 300, 3, 1, 61, 2, 3, 40),
         ("e3", 200, 1, 1, 61, 3, 3, 40)]


def single_long(rows):
    """Iteration's rows (extension: array<long>) as FirstFour holds them (extension: one long)"""
    out = []
    for r in rows:
        e = r.vals[2]
        items = e.items if isinstance(e, jp.Seq) else e
        assert len(items) == 1
        out.append(jp.Row([r.vals[0], r.vals[1], items[0]]))
    return out


def run_case(text_rows, P, stage, start, scramble, passes):
    param = make_param(31, startIteration=start, endIteration=start + passes - 1, scramble=scramble)
    rows = drain(op("it", "DynamicKmerBinarizerFromReducedToSubKmer", param).call(jp.JIter([jp.Row(list(t)) for t in text_rows])))
    assert to_text("it", param, rows) == text_rows                    # the crafted rows are what the reference reads
    which, name = ("ff", "DSExtendReflexivKmer") if stage == 0 else ("it", "DSExtendReflexivKmerToArrayLoop")
    if stage == 0:
        rows = single_long(rows)
    trace = []
    for _ in range(passes):
        rows = run_partitions(which, name, param, rows, P)
        trace.append(to_text(which, param, rows))
    return trace


def main():
    rng = np.random.default_rng(20261020)
    out = {}
    for name, fams, P, stage, start, scramble, passes, ext_max in CASES:
        recs = pymodel.dyn_crafted_families(rng, fams, pymodel.DYN_EDGE_LENGTHS, ext_max)
        text_rows = [(k, f"{m}|{l}|{r}", e) for k, m, e, l, r in recs]
        trace = run_case(text_rows, P, stage, start, scramble, passes)
        out[name + "/meta"] = np.array([P, stage, start, 1 if scramble == 3 else 2, passes], np.int64)
        out[name + "/in"] = pack_rows(text_rows)
        for i, rows in enumerate(trace):
            out[f"{name}/pass{i}"] = pack_rows(rows)
        s = pymodel.dyn_sort(recs)
        _, _, labels = pymodel.dyn_extend_pass(s, pymodel.dyn_partition_starts(s, P), stage, start, 1 if scramble == 3 else 2)
        c = pymodel.dyn_census(labels)
        print(name, len(text_rows), "rows ->", [len(t) for t in trace], "rarest decisions of pass 0:",
              sorted((c.get(lb, 0), lb) for lb in pymodel.dyn_labels(stage, start))[:3], flush=True)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "dynamic_edge_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
