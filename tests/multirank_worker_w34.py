"""One rank of tests/test_gpu_multirank_w34.py: `python multirank_worker_w34.py RANK WORLD WORKDIR` (or `threads WORLD WORKDIR`:
the ranks as threads of this one process), as tests/multirank_worker_w.py, for reads of different lengths at k = RFX_TEST_K
(default 95: three-word k-mers, exchanged as k-mers and counted by the element path).  The
reads are dealt unevenly and the last rank holds none.  Rank 0 checks rfx_dev_sharded_count with per-read lengths against
the one-GPU rfx_dev_count_reads_ragged_w of all the reads, and rfx_sharded_assemble_reads (the extend stage gathered at the
library's default and sharded to the end) against the one-GPU rfx_assemble_reads; then writes WORKDIR/ok<rank>."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

K = int(os.environ.get("RFX_TEST_K", "95"))
W = K // 32 + 1


def main():
    if sys.argv[1] == "threads":
        return main_threads(int(sys.argv[2]), sys.argv[3])
    run_rank(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])


def main_threads(world, work):
    import threading
    import traceback
    import torch
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")                                # one thread makes the process's HIP context
    failed = []

    def body(r):
        try:
            run_rank(r, world, work)
        except BaseException:                                    # noqa: BLE001 -- reported below, with the rank
            failed.append((r, traceback.format_exc()))

    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for r, tb in failed:
        print(f"--- rank {r} of {world} (thread) failed:\n{tb}", flush=True)
    sys.exit(1 if failed else 0)


def share(off, rank, world):
    """reads [a, b) of this rank: the first rank takes half, the others split the rest, the last rank none"""
    n = len(off) - 1
    if world == 1:
        return 0, n
    cuts = [0, n // 2] + [n // 2 + (n - n // 2) * i // (world - 2) for i in range(1, world - 1)] if world > 2 else [0, n, n]
    cuts = cuts[:world] + [n]
    return cuts[rank], cuts[rank + 1]


def run_rank(rank, world, work):
    import torch
    import reflexiv_amd
    from reflexiv_amd import Reflexiv
    from tests.test_gpu_ragged_w import upload
    from tests.test_gpu_count_w34 import ragged_reads_w

    torch.cuda.set_device(0)
    idf = os.path.join(work, "id")
    if rank == 0:
        uid = Reflexiv.comm_unique_id()
        with open(idf + ".tmp", "wb") as f:
            f.write(uid)
        os.rename(idf + ".tmp", idf)
    else:
        t0 = time.time()
        while not os.path.exists(idf):
            assert time.time() - t0 < 300, "rank 0 never published the id"
            time.sleep(0.01)
        uid = open(idf, "rb").read()
    rfx = Reflexiv(0)
    rfx.comm_init(uid, rank, world)

    bases, off = ragged_reads_w(314, K, n_reads=8000, genome_len=20_000)
    a, b = share(off, rank, world)
    mb = np.ascontiguousarray(bases[off[a]:off[b]])
    mo = np.ascontiguousarray(off[a:b + 1] - off[a])
    cover = 2
    dw, dl, n, wpr, maxlen = upload(rfx, torch, mb, mo)
    cap = rfx.kmers_per_read_w(int((off[1:] - off[:-1]).max()), K) * (len(off) - 1)      # (any rank's shard fits: RFX_E_CAP is collective)
    sk = torch.empty(cap * W, dtype=torch.int64, device="cuda"); sc = torch.empty(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ms, tot = rfx.sharded_count_dev(dw.data_ptr(), n, wpr, maxlen, K, sk.data_ptr(), sc.data_ptr(), cap, cover, generations=2,
                                    d_read_len=dl.data_ptr())
    allm = rfx.comm_all_reduce([ms])[0]
    assert allm == tot[2]
    gk = torch.empty(max(1, allm) * W, dtype=torch.int64, device="cuda") if rank == 0 else sk[:0]
    gc = torch.empty(max(1, allm), dtype=torch.int64, device="cuda") if rank == 0 else sc[:0]
    torch.cuda.synchronize()
    got = rfx.gather_shards_dev(sk.data_ptr(), sc.data_ptr(), ms, W, 8, 0, gk.data_ptr(), gc.data_ptr(), allm)
    if rank == 0:
        rfx.order_kmers_w_dev(gk.data_ptr(), gc.data_ptr(), got, K)
        rfx.sync()
        aw, al, an, awpr, amax = upload(rfx, torch, bases, off)
        fcap = rfx.kmers_per_read_w(amax, K) * an
        fk = torch.empty(fcap * W, dtype=torch.int64, device="cuda"); fc = torch.empty(fcap, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        m, nd, inst = rfx.count_reads_ragged_w_dev(aw.data_ptr(), al.data_ptr(), an, awpr, amax, K, fk.data_ptr(), fc.data_ptr(),
                                                   fcap, cover)
        assert tot == [inst, nd, m], ("sharded totals vs one GPU", tot, [inst, nd, m])
        assert got == m and torch.equal(gk[:W * m], fk[:W * m]) and torch.equal(gc[:m], fc[:m])

    prm = reflexiv_amd.default_params(k=K, min_cov=cover, partitions=4, min_contig=100)
    text, nc, trace, tot = rfx.sharded_assemble_reads(mb, mo, prm, generations=2)
    text_s, nc_s, trace_s, tot_s = rfx.sharded_assemble_reads(mb, mo, prm, generations=2, gather_below=0)
    assert (text_s, nc_s, trace_s, tot_s) == (text, nc, trace, tot)
    if rank == 0:
        wtext, wnc, wtrace, kept = rfx.assemble_reads(bases, off, prm)
        assert (text, nc, trace) == (wtext, wnc, wtrace) and nc > 0
    else:
        assert text == "" and nc == 0
    rfx.comm_all_reduce([1])                                   # nobody leaves while a peer still reads its files
    rfx.close()
    with open(os.path.join(work, f"ok{rank}"), "w") as f:
        f.write("ok\n")


if __name__ == "__main__":
    main()
