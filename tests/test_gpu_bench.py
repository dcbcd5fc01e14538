"""bench.py on the GPU as the driver runs it: a plain line carries the count stage only, --steps sets the timed steps, and
--dump-outputs writes the last timed step's survivors -- held to the oracle's count of the same synthetic reads."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs_equal_the_oracle(tmp_path):
    gbp, genome, cover, seed, L, k = 0.01, 200_000, 4, 1, 150, 31
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--gbp", str(gbp),
           "--genome", str(genome), "--cover", str(cover), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "k-mers/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    for extra in ("contigs", "cpu_baseline", "k63", "next_rows", "strong_50gbp"):
        assert extra not in line, extra

    n_reads = int(round(gbp * 1e9 / L))
    n_reads += n_reads & 1
    bases, off = O.synth_reads(seed, O.synth_genome(seed, genome), genome, 0, n_reads, L)
    km = O.extract_canon(bases, off, k)
    wk, wc, wd = O.count_filter(km, cover)
    d = tmp_path / "out"
    summary = np.load(d / "summary.npy")
    assert list(summary[:5]) == [len(wk), wd, len(km), len(wk), int(wc.sum())]
    assert line["config"]["kmer_instances_per_gpu"] == len(km)
    assert line["config"]["kmers_kept"] == len(wk) and line["config"]["distinct_kmers"] == wd
    rows = np.load(d / "rows.npy").astype(np.int64)
    limbs = np.load(d / "keys.npy").astype(np.uint64)
    keys = (limbs[:, 0] << np.uint64(32)) | limbs[:, 1]
    assert np.array_equal(keys, wk.astype(np.uint64)[rows])
    assert np.array_equal(np.load(d / "counts.npy").astype(np.int64), wc.astype(np.int64)[rows])
