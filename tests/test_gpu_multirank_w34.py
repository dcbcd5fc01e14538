"""The multi-GPU branch at k = 95 (three-word k-mers, exchanged as k-mers: the sender buckets them by owner with the count's
level 1, every rank counts its shard with the element path) with reads of different lengths, on several ranks sharing the
one GPU of the test box (RCCL served by tests/fake_rccl, as tests/test_gpu_multirank_w.py).  The reads are dealt unevenly and
one rank holds none; rfx_dev_sharded_count with per-read lengths must give the one-GPU ragged count, and
rfx_sharded_assemble_reads the one-GPU rfx_assemble_reads (tests/multirank_worker_w34.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(HERE, "fake_rccl")
SHIM = os.path.join(SHIM_DIR, "libfake_rccl.so")
WORKER = os.path.join(HERE, "multirank_worker_w34.py")


def build_shim():
    subprocess.run(["make", "-s", "-C", SHIM_DIR], check=True, capture_output=True)
    return SHIM


@pytest.mark.parametrize("world,k", [(2, 95), (3, 95), (2, 124)])
def test_ragged_w34_on_several_ranks(tmp_path, world, k):
    env = dict(os.environ, RFX_RCCL_LIB=build_shim(), HSA_ENABLE_IPC_MODE_LEGACY="0", RFX_TEST_K=str(k))
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), str(tmp_path)], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:                                         # (exactly the processes started here)
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and os.path.exists(tmp_path / f"ok{r}"), f"rank {r} of {world}:\n{o[-3000:]}"
    leftovers = [f for f in os.listdir("/dev/shm") if f.startswith("frccl-")]
    assert not leftovers, leftovers


def test_ragged_k95_world_of_eight_as_threads(tmp_path):
    env = dict(os.environ, RFX_RCCL_LIB=build_shim(), HSA_ENABLE_IPC_MODE_LEGACY="0", FAKE_RCCL_TIMEOUT_S="120", RFX_TEST_K="95")
    p = subprocess.run([sys.executable, WORKER, "threads", "8", str(tmp_path)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0 and all(os.path.exists(tmp_path / f"ok{r}") for r in range(8)), p.stdout[-4000:]
    leftovers = [f for f in os.listdir("/dev/shm") if f.startswith("frccl-")]
    assert not leftovers, leftovers
