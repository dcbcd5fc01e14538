"""bench.py's command line on the CPU: a plain run times the count stage only (--full adds the other blocks), and
--dump-outputs writes the step's output exactly (32-bit limbs in float64), bounded in size, sampled the same way each time."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

EXTRAS = ("no_cpu_baseline", "no_contigs", "no_k63", "no_ingest", "no_next_rows", "no_strong")


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_skips_every_extra_block(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert all(getattr(a, f) for f in EXTRAS)


def test_full_run_keeps_the_extra_blocks_and_their_switches(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--full")
    assert not any(getattr(a, f) for f in EXTRAS)
    a = parse(monkeypatch, "--gpus", "1", "--full", "--no-k63", "--no-strong", "--dump-outputs", "d")
    assert a.no_k63 and a.no_strong and not a.no_contigs and not a.no_cpu_baseline and a.dump_outputs == "d"


@pytest.mark.parametrize("W,n,budget", [(1, 5000, 1 << 20), (1, 5000, 40_000), (2, 3000, 50_000), (1, 0, 1 << 20)])
def test_dump_outputs_exact_bounded_and_repeatable(monkeypatch, tmp_path, W, n, budget):
    import torch
    monkeypatch.setattr(bench, "DUMP_BYTES", budget)
    rng = np.random.default_rng(W * 1000 + n)
    words = np.sort(rng.integers(0, 1 << 62, size=(n, W), dtype=np.int64), axis=0)
    counts = rng.integers(2, 1 << 20, size=n, dtype=np.int64)
    keys_t, counts_t = torch.from_numpy(words.reshape(-1).copy()), torch.from_numpy(counts.astype(np.int32 if W == 1 else np.int64))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), keys_t, counts_t, W, n, 3 * n, 9 * n, 0, 1)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["counts.npy", "keys.npy", "rows.npy", "summary.npy"]
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(v.dtype == np.float64 for v in got.values())
    for f in files:                                            # the same arguments give the same files
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f)), f
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget + 4096
    rows = got["rows.npy"].astype(np.int64)
    assert len(rows) == (n if n * 8 * (2 * W + 2) <= budget else budget // (8 * (2 * W + 2)))
    assert np.all(np.diff(rows) > 0) and (len(rows) == 0 or rows[-1] < n)
    limbs = got["keys.npy"].astype(np.uint64)
    assert limbs.shape == (len(rows), 2 * W)
    back = (limbs[:, 0::2] << np.uint64(32)) | limbs[:, 1::2]
    assert np.array_equal(back, words.view(np.uint64)[rows])
    assert np.array_equal(got["counts.npy"].astype(np.int64), counts[rows])
    s = got["summary.npy"]
    xor = np.bitwise_xor.reduce(words.view(np.uint64), axis=0) if n else np.zeros(W, np.uint64)
    want_xor = [int(x >> np.uint64(32)) for x in xor], [int(x & np.uint64(0xFFFFFFFF)) for x in xor]
    assert list(s[:5]) == [n, 3 * n, 9 * n, n, int(counts.sum())]
    assert [int(x) for x in s[5:]] == [v for pair in zip(*want_xor) for v in pair]
