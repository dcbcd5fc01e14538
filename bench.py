#!/usr/bin/env python3
"""bench.py -- k-mers/sec of the count stage (extract + count + filter) on synthetic PE150
reads, k = 31, with the kernel roofline and the CPU baseline beside it.

    python bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path's count stage over one batch of synthetic reads that is
already resident in HBM (2-bit packed): at N = 1 the batch is BASELINE.json configs[1]
("Synthetic 5 Gbp E.coli-like PE150, k=31, 1xMI355X": 33,333,334 reads of 150 bp from a
4.64 Mbp genome, 0.5 % substitutions, -cover 30).  At N > 1 every rank holds its own 6.25 Gbp
shard of the read set (weak scaling; 8 x 6.25 = the 50 Gbp of BASELINE configs[2] and of the
metric), k-mer space is radix-sharded over the ranks and one RCCL all-to-all(v) replaces the
Spark shuffle.  Run without a launcher, `--gpus N` starts its own N ranks (torch.distributed.run)
and refuses to run when fewer than N GPUs are visible.

A plain run sets up, warms up, times the K steps and prints the line.  With --full the run also
measures everything else the line can carry: the CPU baseline, the wall-clock to final contigs
(and the de-duplication, the ASCII ingest, the k = 63 block, the `next_rows` and `strong_50gbp`
blocks at N = 1).  --dump-outputs DIR writes what the last timed step computed (the surviving
k-mers and their counts; a fixed, seeded sample of them when they are many) as .npy files.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# functional rehearsal of the N > 1 branch on a ONE-GPU box (tests/test_gpu_multirank.py): every rank on cuda:0, gloo for
# torch's own collectives, the C ABI's RCCL served by the tests' stand-in (RFX_RCCL_LIB); the line says so ("rehearsal")
SHARED_GPU = os.environ.get("RFX_BENCH_SHARED_GPU", "0") == "1" and bool(os.environ.get("RFX_RCCL_LIB"))
HBM_PEAK_GBPS = 8000.0        # MI355X HBM3E peak (MI355X_MICROARCH.md: 8 TB/s spec)

# algorithmic HBM bytes per k-mer instance, per kernel family (DESIGN.md "Kernels")
ALGO_BYTES = {"hist1": 0.25, "part1": 8.25, "hist2": 8.0, "part2": 16.0, "hist3": 8.0, "part3": 16.0,
              "leaf": 8.0, "extract_w": 0.25 + 16.0, "count_w": 16.0}      # k = 63: W = 2 words per instance


TRAFFIC_PROFILES = ("profiles/r04_hbm_traffic.json", "profiles/r03_hbm_traffic.json", "profiles/r02_hbm_traffic.json", "profiles/r01_hbm_traffic.json")


def measured_traffic(kernel, n_inst):
    """HBM bytes per launch of `kernel` from a COMMITTED PMC profile of this same command (rocprofv3 --pmc, separate
    FETCH_SIZE / WRITE_SIZE passes, FETCH doubled per MI355X_MICROARCH.md) when one exists for this workload.  PMC
    counters cannot be read from inside the run, so this is evidence from the builder's box, named as such in
    `traffic_source`; (None, None) when no profile matches.  -> (bytes per launch, source)"""
    for rel in TRAFFIC_PROFILES:
        try:
            prof = json.load(open(os.path.join(ROOT, rel)))
            if prof.get("kmer_instances") == n_inst and kernel in prof["kernels"]:
                return prof["kernels"][kernel]["hbm_bytes_per_launch"], \
                    rel + " (rocprofv3 --pmc passes of this command on the builder's box; not measured in this run)"
        except (OSError, ValueError, KeyError):
            pass
    return None, None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gbp", type=float, default=None,
                    help="Gbp of reads per GPU (default: 5 at N = 1 = BASELINE configs[1]; 6.25 at N > 1, i.e. the 50 Gbp of "
                         "BASELINE configs[2] / the metric at 8 GPUs, the same per-GPU work at 2 and 4)")
    ap.add_argument("--genome", type=int, default=None,
                    help="genome length (bases, multiple of 32).  Default: 4,640,000 per 5 Gbp of TOTAL reads -- the E.coli-like genome "
                         "of BASELINE configs[1] at N = 1, and the SAME DEPTH (1078x, -cover 30) at every N: 46.4 Mbp for the 50 Gbp of 8 "
                         "GPUs.  (With one 4.64 Mbp genome at every N the depth per site grows with N -- 10776x at 8 GPUs -- and with it "
                         "the work per k-mer instance: every minimiser site then brings ~9500 records, more than one LDS table takes, "
                         "measured 8.0 ns per 1000 instances in the leaves against 2.2 at 1078x; per-GPU work would not be fixed as N "
                         "grows, which is what weak scaling means.  --genome 4640000 selects that set.)")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--cover", type=int, default=None,
                    help="-cover (minKmerCoverage); default 30 per 5 Gbp of TOTAL reads on the 4.64 Mbp genome (error k-mers "
                         "recur in proportion to the depth: 30 at 1078x, 300 at 10776x)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--partitions", type=int, default=8)
    ap.add_argument("--cpu-sample-reads", type=int, default=4_000_000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-contigs", action="store_true")
    ap.add_argument("--no-k63", action="store_true", help="N = 1, k = 31: skip the second block (the same reads at k = 63)")
    ap.add_argument("--no-ingest", action="store_true",
                    help="N = 1: skip contigs.wall_ms_ascii_to_contigs (rfx_assemble_reads from pinned host ASCII)")
    ap.add_argument("--force-dist", action="store_true",
                    help="run the multi-GPU code path (owner buckets, RCCL all-to-all, gather) even with one rank")
    ap.add_argument("--exchange-chunks", type=int, default=4,
                    help="N > 1: read chunks whose all-to-all overlaps the bucketing of the next chunk (1 = no overlap)")
    ap.add_argument("--exchange", choices=["auto", "pairs", "records"], default="auto",
                    help="N > 1, k <= 31: what crosses the all-to-all -- (k-mer, local count) pairs after a local combine "
                         "(reduceByKey's map-side combine: fewer bytes at high coverage, the local count hides the flight) or "
                         "super-k-mer records in --generations of the hash space (less compute; the count of one generation "
                         "hides the flight of the next).  auto: records (since round 2 the form with less compute at every N; pairs stay selectable)")
    ap.add_argument("--generations", type=int, default=4, help="--exchange records: generations of the hash space")
    ap.add_argument("--virtual-world", type=int, default=8,
                    help="--force-dist on one rank: bucket the reads as a rank of this many GPUs would (generations x owners bins) "
                         "and count per generation what such a rank would receive -- the per-rank kernel work of an N-GPU step "
                         "without the links (RFX_COMM_VIRTUAL_WORLD)")
    ap.add_argument("--exchange-impl", choices=["capi", "torch"], default="capi",
                    help="N > 1, --exchange records: capi = rfx_dev_sharded_count (RCCL send / recv inside libreflexiv_hip.so, "
                         "the form a Java / C host calls); torch = reflexiv_amd.dist over torch.distributed")
    ap.add_argument("--strong", action="store_true",
                    help="strong scaling on north_star's 50 Gbp read set: the SAME 333,333,334 reads at every N (50 / N Gbp per GPU, "
                         "-cover 300); N = 1 counts them in --strong-generations sequential generations of the hash space through "
                         "rfx_dev_sharded_count on a one-rank communicator (nothing travels, nothing is copied).  The JSON line says "
                         '"scaling": "strong".  Without the flag the N = 1 line carries the same measurement as `strong_50gbp` '
                         "(few steps), the denominator a weak-scaled N = 8 line -- 8 x 6.25 Gbp = the same 50 Gbp -- is read against")
    ap.add_argument("--strong-generations", type=int, default=8)
    ap.add_argument("--no-strong", action="store_true", help="N = 1: skip the strong_50gbp block")
    ap.add_argument("--no-next-rows", action="store_true",
                    help="N = 1: skip the `next_rows` block (SURVEY.md 8f-2 / f-4 at scale: the dynamic-k passes on 10^7 rows, the contig RC "
                         "de-duplication of 10^5 contigs; tools/bench_f2f4.py)")
    ap.add_argument("--gather-below", type=int, default=0,
                    help="--sharded-extend: the record set is gathered on rank 0 once it has this many records or fewer over all "
                         "ranks (0: the whole loop stays sharded; -1: the library's default, 32 Mi)")
    ap.add_argument("--sharded-extend", action="store_true",
                    help="N > 1 (or --force-dist): run the extend stage range-sharded over the ranks with the records resident "
                         "in HBM (reflexiv_amd.dist.sharded_assemble_dev: one RCCL all-to-all of whole records per sortByKey) "
                         "instead of gathering the survivors on rank 0 -- what a genome beyond one GPU needs; k <= 31")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the count stage too: CPU baseline, contigs (dedup, ASCII ingest), k = 63, "
                         "next_rows, strong_50gbp.  Without it the run times the count stage only (the --no-* flags select "
                         "within --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float64): the surviving "
                         "k-mers as 32-bit limbs, their counts, and a summary with checksums over all of them")
    args = ap.parse_args()
    if not args.full:
        args.no_cpu_baseline = args.no_contigs = args.no_k63 = args.no_ingest = args.no_next_rows = args.no_strong = True
    if args.strong:
        args.gbp = 50.0 / args.gpus
        if args.gpus == 1:
            args.force_dist, args.virtual_world, args.generations = True, 1, args.strong_generations
            args.no_k63 = args.no_ingest = args.no_cpu_baseline = True
    if args.gbp is None:
        args.gbp = 5.0 if args.gpus == 1 else 6.25
    if args.genome is None:
        args.genome = int(round(4_640_000 * args.gbp * args.gpus / 5.0 / 32)) * 32 if args.gpus > 1 or args.strong else 4_640_000
    if args.cover is None:
        args.cover = max(2, int(round(30 * args.gbp * args.gpus / 5.0 * 4_640_000 / args.genome)))
    return args


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks ourselves as a
    child `torch.distributed.run` (one process per GPU, RCCL rendezvous on 127.0.0.1) BEFORE this process
    touches the GPU, and exit with the child's code."""
    import subprocess
    import torch
    have = torch.cuda.device_count()            # does not initialise the GPU runtime
    if have < args.gpus and not SHARED_GPU:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} asked for, {have} GPU(s) visible on this box: refusing to run "
                         f"(a {args.gpus}-GPU number can only come from {args.gpus} ranks)\n")
        sys.exit(2)
    port = os.environ.get("MASTER_PORT", str(29500 + os.getpid() % 2000))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.run(cmd).returncode)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(args, n_sample, n_reads_total):
    """The oracle (CPU restatement of the same operators) over ALL host cores, OpenMP, one logical partition per
    task (SURVEY.md 8d / BASELINE.md 3: "reference-equivalent CPU path (C restatement), not Spark/JVM"), on a bounded
    sample of the same workload -- the first n_sample reads -- through the WHOLE path: extract + count + filter
    (k-mers/s) and on to final contigs (wall-clock).  -cover is scaled to the sample's depth."""
    import numpy as np
    from oracle import oracle as O
    cores = O.host_cores()
    O.set_threads(cores)
    cover = max(2, int(round(args.cover * n_sample / n_reads_total)))
    g = O.synth_genome(args.seed, args.genome)
    bases, off = O.synth_reads(args.seed, g, args.genome, 0, n_sample, args.read_len)
    t0 = time.perf_counter()
    keys, counts, nd, n = O.count_reads_omp(bases, off, args.k, cover, 10_000_000, 0,
                                            cap=max(1 << 20, 4 * args.genome))
    t_count = time.perf_counter() - t0
    # one logical partition per host thread (the extend loop is a task per partition: at the GPU run's 8 partitions
    # it would leave 248 of a GPU box's 256 cores idle)
    p_cpu = max(args.partitions, min(cores, 1024))
    prm = O.default_params(k=args.k, min_cov=cover, partitions=p_cpu)
    t1 = time.perf_counter()
    text, nc, trace, _ = O.assemble_from_counts(keys, counts, prm)
    t_asm = time.perf_counter() - t1
    O.set_threads(1)
    lens = sorted((int(h.split("-")[1]) for h in text.split("\n") if h.startswith(">")), reverse=True)
    return {"value": n / t_count, "unit": "k-mers/s", "cores": cores, "kind": "port", "cpu_model": cpu_model(),
            "label": "reference-equivalent CPU path (C restatement of the Spark operators, OpenMP, one logical partition "
                     "per task), not Spark/JVM",
            "sample": f"first {n_sample} reads of the workload ({n} k-mer instances, {n_sample * args.read_len / args.genome:.0f}x, "
                      f"-cover {cover}): extract+count+filter {t_count:.2f} s, counts -> contigs {t_asm:.2f} s "
                      f"({len(trace)} extend passes, {p_cpu} logical partitions), on {cores} host cores "
                      "(oracle/reflexiv_oracle.c, orc_count_reads_omp + orc_assemble_from_counts)",
            "count_stage_s": t_count, "counts_to_contigs_s": t_asm, "reads_to_contigs_s": t_count + t_asm,
            "kmers_kept": int(len(keys)), "distinct_kmers": int(nd), "n_contigs": nc, "longest": lens[:3]}


def k63_block(args, rfx, torch, reflexiv_amd, d_words, n_reads, wpr, L, dev):
    k = 63
    W = 2
    n_inst = rfx.kmers_per_read_w(L, k) * n_reads
    cap = max(1 << 20, n_inst // 8)
    d_keys = torch.empty(cap * W, dtype=torch.int64, device=dev)
    d_counts = torch.empty(cap, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def step():
        return rfx.count_reads_w_dev(d_words.data_ptr(), n_reads, wpr, L, k, d_keys.data_ptr(), d_counts.data_ptr(), cap, args.cover)
    for _ in range(max(1, args.warmup)):
        step()
    torch.cuda.synchronize()
    acc = {}
    t0 = time.perf_counter()
    for _ in range(args.steps):
        m, nd, inst = step()
        for name, (ms, ln) in rfx.count_timing().items():
            a = acc.setdefault(name, [0.0, 0]); a[0] += ms; a[1] += ln
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    leaf_ms = acc.get("leaf", [0.0])[0] / args.steps
    prm = reflexiv_amd.default_params(k=k, min_cov=args.cover, partitions=args.partitions)
    aw = (k - 1) // 31 + 1
    a_k = torch.empty(max(1, m) * aw, dtype=torch.int64, device=dev)
    a_c = torch.empty(max(1, m), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def assemble():
        m2 = rfx.counter_to_asm_dev(d_keys.data_ptr(), d_counts.data_ptr(), m, k, a_k.data_ptr(), a_c.data_ptr(), args.cover)
        return rfx.assemble_w_dev(a_k.data_ptr(), a_c.data_ptr(), m2, prm)
    assemble()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    text, nc, trace = assemble()
    t_asm = time.perf_counter() - t1
    lens = sorted((int(h.split("-")[1]) for h in text.split("\n") if h.startswith(">")), reverse=True)
    return {"k": k, "dtype": "2 x u64", "kmer_instances": n_inst, "distinct_kmers": nd, "kmers_kept": m,
            "ms_per_step": dt * 1e3, "value": n_inst / dt, "unit": "k-mers/s", "steps": args.steps,
            "stage_hbm_frac": ((0.25 + 16 * W) * n_inst + (8 * W + 4) * m) / dt / 1e9 / HBM_PEAK_GBPS,
            "leaf_ms": leaf_ms, "leaf_roofline_frac": (8 * W * n_inst / (leaf_ms / 1e3) / 1e9 / HBM_PEAK_GBPS) if leaf_ms else None,
            "per_kernel_ms_per_step": {n: v[0] / args.steps for n, v in sorted(acc.items()) if not n.startswith("stat_")},
            "contigs": {"wall_ms_from_counts": t_asm * 1e3, "wall_ms_reads_to_contigs": t_asm * 1e3 + dt * 1e3, "extend_passes": len(trace),
                        "n_contigs": nc, "longest": lens[:3], "total_bases": sum(lens)}}


def strong_block(args, rfx, torch, reflexiv_amd, dev):
    """north_star's strong-scaling denominator: the 50 Gbp read set (333,333,334 PE150 reads, -cover 300 -- what 8 GPUs x 6.25
    Gbp hold between them) counted on ONE GPU in G sequential generations of the hash space (rfx_dev_sharded_count on a
    one-rank communicator: bucketed once by generation, each generation counted where it lies).  8-GPU efficiency =
    value of the N = 8 line / (8 x this value)."""
    L, k, G = args.read_len, args.k, args.strong_generations
    wpr = (L + 31) // 32
    n_reads = int(round(50e9 / L))
    n_reads += n_reads & 1
    genome = 46_400_000 if not args.strong else args.genome       # the depth of configs[1]: what `--gpus 8` counts by default
    cover = max(2, int(round(30 * 50.0 / 5.0 * 4_640_000 / genome)))
    n_inst = rfx.kmers_per_read(L, k) * n_reads
    d_genome = torch.empty((genome + 31) // 32, dtype=torch.int64, device=dev)
    d_words = torch.empty(n_reads * wpr, dtype=torch.int64, device=dev)
    cap = max(1 << 24, 2 * genome)
    d_keys = torch.empty(cap, dtype=torch.int64, device=dev)
    d_counts = torch.empty(cap, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rfx.synth_genome_dev(args.seed, genome, d_genome.data_ptr())
    rfx.synth_reads_dev(args.seed, d_genome.data_ptr(), genome, 0, n_reads, L, wpr, d_words.data_ptr())
    rfx.sync()
    made = not getattr(rfx, "comm", None)
    if made:
        rfx.comm_init(reflexiv_amd.Reflexiv.comm_unique_id(), 0, 1)
    old = os.environ.pop("RFX_COMM_VIRTUAL_WORLD", None)
    try:
        def step():
            return rfx.sharded_count_dev(d_words.data_ptr(), n_reads, wpr, L, k, d_keys.data_ptr(), d_counts.data_ptr(), cap, cover, generations=G)
        step()
        torch.cuda.synchronize()
        steps = 3
        t0 = time.perf_counter()
        for _ in range(steps):
            m, tot = step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        tm = {n: ms for n, (ms, ln) in rfx.count_timing().items() if not n.startswith("stat_")}
    finally:
        if old is not None:
            os.environ["RFX_COMM_VIRTUAL_WORLD"] = old
        if made:
            rfx.comm_destroy()
    rfx.trim()
    return {"workload": f"synthetic 50 Gbp, genome {genome} bp (1078x, the depth of configs[1]), PE{L}, k={k}, -cover {cover}: the read set of N = 8 x 6.25 Gbp",
            "n_gpus": 1, "reads": n_reads, "kmer_instances": n_inst, "generations": G, "distinct_kmers": tot[1], "kmers_kept": tot[2],
            "steps": steps, "ms_per_step": dt * 1e3, "value": n_inst / dt, "unit": "k-mers/s",
            "per_kernel_ms_last_step": tm,
            "how_to_read": "strong-scaling efficiency at N GPUs on this read set = value(N-GPU line, N x 50/N Gbp) / (N x this value); "
                           "north_star asks >= 6x at N = 8, i.e. value(N = 8) >= 6 x this value"}


DUMP_BYTES = 56 << 20          # --dump-outputs: at most this much per rank (the files stay under 64 MB in all at N = 1)


def dump_outputs(path, keys, counts, W, m, nd, inst, rank, world):
    """The last timed step's output (ascending k-mers, W words each, and their counts) as float64 .npy files: keys.npy holds
    each k-mer as 2W 32-bit limbs (most significant first: exact in float64), counts.npy its count, rows.npy the row of each;
    when the rows exceed DUMP_BYTES they are a fixed, seeded sample.  summary.npy: kept, distinct, instances, this rank's
    rows, the sum of all counts and the XOR of all key words (as 32-bit limbs) over every row, sampled or not."""
    import numpy as np
    k64 = keys.contiguous().cpu().numpy().view(np.uint64).reshape(-1, W)
    c = counts.contiguous().cpu().numpy().astype(np.int64)
    n = len(c)
    assert k64.shape[0] == n, (k64.shape, n)
    limbs = np.empty((n, 2 * W), np.uint64)
    limbs[:, 0::2], limbs[:, 1::2] = k64 >> np.uint64(32), k64 & np.uint64(0xFFFFFFFF)
    per_row = 8 * (2 * W + 2)
    rows = np.arange(n)
    if n * per_row > DUMP_BYTES:
        rows = np.sort(np.random.default_rng(20261016).choice(n, DUMP_BYTES // per_row, replace=False))
    xor = np.bitwise_xor.reduce(limbs, axis=0) if n else np.zeros(2 * W, np.uint64)
    sfx = f"_rank{rank}" if world > 1 else ""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, f"keys{sfx}.npy"), limbs[rows].astype(np.float64))
    np.save(os.path.join(path, f"counts{sfx}.npy"), c[rows].astype(np.float64))
    np.save(os.path.join(path, f"rows{sfx}.npy"), rows.astype(np.float64))
    np.save(os.path.join(path, f"summary{sfx}.npy"),
            np.array([m, nd, inst, n, int(c.sum())] + [int(x) for x in xor], np.float64))


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)                                     # never returns
    import torch
    import torch.distributed as dist
    import reflexiv_amd
    from reflexiv_amd import dist as rd

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = 0 if SHARED_GPU else int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks\n")
        sys.exit(2)
    if not torch.cuda.is_available() or torch.cuda.device_count() <= local:
        sys.stderr.write("bench.py needs one MI355X per rank (no CPU fallback)\n")
        sys.exit(2)
    torch.cuda.set_device(local)
    multi = world > 1 or args.force_dist
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29577")
        if SHARED_GPU:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        # n_gpus in the JSON line is what RCCL saw, nothing else
        world = dist.get_world_size()
        probe = torch.ones(1, device="cpu" if SHARED_GPU else torch.device("cuda", local))
        dist.all_reduce(probe)
        if int(probe.item()) != args.gpus and not (args.force_dist and args.gpus == 1):
            sys.stderr.write(f"bench.py: {int(probe.item())} ranks joined the RCCL group, --gpus {args.gpus} asked for\n")
            sys.exit(2)
    L, k = args.read_len, args.k
    wpr = (L + 31) // 32
    n_reads = int(round(args.gbp * 1e9 / L))
    n_reads += n_reads & 1                                    # whole pairs
    # the CPU baseline runs FIRST (rank 0, N = 1, k <= 31 only), before anything touches the GPU: the GPU phase of
    # the run is then one uninterrupted stretch at the end
    cpu_record = None
    if rank == 0 and not multi and not args.no_cpu_baseline and k <= 31:
        cpu_record = cpu_baseline(args, min(args.cpu_sample_reads, n_reads), n_reads)
    rfx = reflexiv_amd.Reflexiv(local)
    rfx.use_stream(torch.cuda.current_stream().cuda_stream)   # kernels, copies and RCCL share one stream
    dev = torch.device("cuda", local)

    wide = k > 31                                             # the counter's multi-word k-mers
    W = k // 32 + 1 if wide else 1
    nk = rfx.kmers_per_read_w(L, k) if wide else rfx.kmers_per_read(L, k)
    n_inst = nk * n_reads                                     # instances per rank per step
    if wide:
        args.no_cpu_baseline = True

    # synthetic reads straight into HBM, 2-bit packed (data = "synthetic")
    d_genome = torch.empty((args.genome + 31) // 32, dtype=torch.int64, device=dev)
    d_words = torch.empty(n_reads * wpr, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    rfx.synth_genome_dev(args.seed, args.genome, d_genome.data_ptr())
    rfx.synth_reads_dev(args.seed, d_genome.data_ptr(), args.genome, rank * n_reads, n_reads, L, wpr,
                        d_words.data_ptr())
    rfx.sync()

    cap = max(1 << 20, n_inst // 8)
    d_keys = torch.empty(cap * W, dtype=torch.int64, device=dev)
    d_counts = torch.empty(cap, dtype=torch.int64 if wide else torch.int32, device=dev)
    reads = dict(words=d_words, n_reads=n_reads, wpr=wpr, read_len=L, k=k)
    if args.exchange == "auto":
        args.exchange = "records"
    engine = rd.HipEngine(rfx, combine=args.exchange == "pairs" and not wide)
    engine.force_exchange = args.force_dist
    capi = multi and args.exchange == "records" and args.exchange_impl == "capi" and (3 <= k <= 125 and k % 32 != 0)
    if capi:
        if world == 1 and args.force_dist and args.virtual_world > 1:
            os.environ["RFX_COMM_VIRTUAL_WORLD"] = str(args.virtual_world)
        # the RCCL communicator of the C ABI: rank 0 makes the id, torch.distributed only carries its 128 bytes
        box = [reflexiv_amd.Reflexiv.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        rfx.comm_init(box[0], rank, world)
    if args.force_dist and world == 1 and not capi:
        # one-rank rehearsal: the rank's own bucket is handed over by a device copy, i.e. the numbers of this
        # mode contain NO exchange time (labelled "exchange_free" in the JSON line)
        rd.LOCAL_SHORTCUT = True
    timing_acc = {}

    shard = {}
    # enough chunks that no per-peer message needs the staged rounds of dist._alltoallv (512 MiB cap);
    # pairs: 16 B per distinct k-mer of a chunk: 1.4 B per instance unchunked, 2.3 B in 8 chunks on this workload
    per_inst = (5.6 if engine.wide_records else 16.0) if wide else 2.6 if engine.combine else 2.7
    est_chunks = per_inst * n_inst / world / rd.A2A_LIMIT_BYTES

    def step():
        if wide and not multi:
            return rfx.count_reads_w_dev(d_words.data_ptr(), n_reads, wpr, L, k, d_keys.data_ptr(), d_counts.data_ptr(),
                                         cap, args.cover)
        if not multi:
            m, nd, inst = rfx.count_reads_dev(d_words.data_ptr(), n_reads, wpr, L, k, d_keys.data_ptr(),
                                              d_counts.data_ptr(), cap, args.cover)
            return m, nd, inst
        est = est_chunks
        chunks = max(args.exchange_chunks, int(est) + 1)
        gens = args.generations if (args.exchange == "records" and (capi or not wide)) else 1
        while gens > 1 and world * gens > 64:
            gens //= 2
        if capi:
            m, tot = rfx.sharded_count_dev(d_words.data_ptr(), n_reads, wpr, L, k, d_keys.data_ptr(), d_counts.data_ptr(), cap,
                                           args.cover, generations=gens)
            shard["keys"], shard["counts"] = d_keys[:m * W], d_counts[:m]
            engine.bucketed_bytes = getattr(engine, "bucketed_bytes", 0) + rfx.comm_bytes_bucketed()
            for name, (ms, ln) in rfx.count_timing().items():
                a = engine.timing.setdefault(name, [0.0, 0])
                a[0] += ms; a[1] += ln
            return tot[2], tot[1], tot[0] // world
        keys, counts, tot = rd.sharded_count(engine, reads, args.cover, 10_000_000, 0, chunks=chunks, generations=gens)
        shard["keys"], shard["counts"] = keys, counts
        return tot[2], tot[1], tot[0] // world

    def sync_all():
        torch.cuda.synchronize()
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    # N > 1: one extra untimed step ahead of the W warm-up steps (disclosed as "extra_untimed_steps"): the
    # first step creates the RCCL communicator and settles every grow-only buffer, and on a fresh box the
    # second one still pages code in (tools/prof_dist.py: 400 / 185 / 63 ms for steps 0 / 1 / 2)
    extra_untimed = 1 if multi else 0
    for _ in range(args.warmup + extra_untimed):
        step()
    sync_all()
    engine.bucketed_bytes = 0
    t0 = time.perf_counter()
    for _ in range(args.steps):
        engine.timing.clear()
        m, nd, inst = step()
        # N = 1: the one fused call; N > 1: every library call of the step (the engine adds them up)
        for name, (ms, ln) in (engine.timing if multi else {n: list(v) for n, v in rfx.count_timing().items()}).items():
            a = timing_acc.setdefault(name, [0.0, 0])
            a[0] += ms; a[1] += ln
    sync_all()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64, device="cpu" if SHARED_GPU else dev)
    if multi:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    total_inst = n_inst * world * args.steps
    value = total_inst / dt

    # roofline of the dominant kernel family: algorithmic bytes per launch / average launch
    # duration (HIP events recorded inside the library on the stream the kernels run on)
    roofline = None
    if timing_acc:
        dom = max((n for n in timing_acc if n in ALGO_BYTES), key=lambda n: timing_acc[n][0])
        ms, launches = timing_acc[dom]
        per_launch_bytes = ALGO_BYTES[dom] * n_inst
        # a step may launch the family more than once (heavy leaves are counted in a second launch; N > 1 runs
        # it over parts of the batch): price the family's time per STEP against the batch's algorithmic bytes
        avg_s = ms / 1e3 / args.steps
        achieved = per_launch_bytes / avg_s / 1e9
        traffic, traffic_source = measured_traffic(dom, n_inst)
        roofline = {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": traffic_source,
                    "algorithmic_bytes_per_launch": per_launch_bytes, "avg_launch_ms": avg_s * 1e3,
                    "launches_per_step": launches / args.steps,
                    "per_kernel_ms_per_step": {n: v[0] / args.steps for n, v in sorted(timing_acc.items()) if not n.startswith("stat_")}}

    out = {
        "metric": "k-mers/sec (extract+count+filter; wall-clock to final contigs beside it)",
        "value": value, "unit": "k-mers/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong" if args.strong else "weak", "extra_untimed_steps": extra_untimed,
        "vs_baseline": None, "dtype": "u64", "data": "synthetic",
        "config": {"workload": f"synthetic {args.gbp * world:g} Gbp in all ({args.gbp:g} Gbp per GPU x {world}), "
                               f"{'E.coli-like ' if args.genome == 4_640_000 else ''}genome {args.genome} bp "
                               f"({args.gbp * world * 1e9 / args.genome:.0f}x), PE{L}, k={k}, -cover {args.cover}, 0.5% substitutions",
                   "reads_per_gpu": n_reads, "kmer_instances_per_gpu": n_inst, "distinct_kmers": nd,
                   "kmers_kept": m,
                   "parallelism": "1 GPU" if not multi else f"k-mer space radix-sharded over {world} GPUs, "
                                                               "RCCL all-to-all(v) of " +
                                                               (f"32-byte super-k-mer records of two-word k-mers{', ' + str(args.generations) + ' generations' if capi else ''}" if wide
                                                                else "(k-mer, local count) pairs"
                                                                if engine.combine else f"super-k-mer records, {args.generations} generations")},
        "roofline": roofline,
        "stage_hbm_frac": (((0.25 + 16 * W) * n_inst + (8 * W + 4) * m) / (dt / args.steps) / 1e9 / HBM_PEAK_GBPS) if not multi else None,
    }

    if SHARED_GPU:
        out["rehearsal"] = (f"FUNCTIONAL REHEARSAL, not a measurement: {world} ranks share ONE GPU, RCCL replaced by the tests' "
                            "stand-in (RFX_BENCH_SHARED_GPU / RFX_RCCL_LIB); the timing fields mean nothing")
    if multi:
        # what crosses the all-to-all: every rank buckets B bytes per step and keeps 1/N of them; each
        # peer's share travels over its own xGMI link (7 links x ~153 GB/s per GPU, MI355X_MICROARCH.md)
        B = engine.bucketed_bytes / args.steps
        out["exchange"] = {"unit": out["config"]["parallelism"].split(" of ")[-1], "bytes_bucketed_per_gpu_per_step": B,
                           "bytes_per_instance": B / n_inst, "bytes_leaving_per_gpu_per_step": B * (world - 1) / world,
                           "per_link_floor_ms_at_153GBps": B / world / 153e9 * 1e3 if world > 1 else 0.0,
                           "chunks": 1 if (args.exchange == "records" and not wide) else max(args.exchange_chunks, int(est_chunks) + 1),
                           "impl": "rfx_dev_sharded_count (RCCL send/recv inside libreflexiv_hip.so)" if capi
                                   else "reflexiv_amd.dist over torch.distributed",
                           "exchange_free": bool((rd.LOCAL_SHORTCUT or capi) and world == 1),
                           "rehearsed_as_rank_of": args.virtual_world if (capi and world == 1 and args.force_dist) else None}
    if args.dump_outputs:
        keys_out, counts_out = (shard["keys"], shard["counts"]) if multi else (d_keys[:m * W], d_counts[:m])
        dump_outputs(args.dump_outputs, keys_out, counts_out, W, m, nd, inst, rank, world)
    if multi and not args.no_contigs and capi:
        # the extend stage behind the C ABI (rfx_dev_sharded_assemble): every sortByKey of the driver is a range shuffle of whole
        # records over the ranks while the record set has more than gather_below records (the library's 32 Mi unless
        # --sharded-extend names one), then rank 0 finishes -- a bacterial genome's survivors go to rank 0 at once
        gather_below = args.gather_below if args.sharded_extend else -1
        prm = reflexiv_amd.default_params(k=k, min_cov=args.cover, partitions=args.partitions)
        sk, sc = shard["keys"].contiguous(), shard["counts"].contiguous()
        ms = int(sc.numel())
        if wide:                                              # KmerBinarizer on the shard (counter layout -> assembler layout)
            aw = (k - 1) // 31 + 1
            a_k = torch.empty(max(1, ms) * aw, dtype=torch.int64, device=dev)
            a_c = torch.empty(max(1, ms), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ms = rfx.counter_to_asm_dev(sk.data_ptr(), sc.data_ptr(), ms, k, a_k.data_ptr(), a_c.data_ptr(), args.cover)
            sk, sc = a_k, a_c
        torch.cuda.synchronize()
        text, nc, tr, t_asm, asm_error = "", 0, [], 0.0, None
        # a watchdog: the count stage's line must not be lost over the extend stage.  More than one rank with real RCCL runs
        # here for the first time on the driver's 8-GPU node (the build pool has one GPU per session): if the collective path
        # does not come back within RFX_BENCH_EXTEND_TIMEOUT_S, rank 0 prints the line with the timeout recorded and every
        # rank leaves.
        import threading

        def bail():
            if rank == 0:
                out["contigs"] = {"error": "the multi-GPU extend stage did not return within the bench's watchdog time; the count-stage "
                                           "fields of this line are complete"}
                print(json.dumps(out), flush=True)
            os._exit(0 if rank == 0 else 3)
        dog = threading.Timer(float(os.environ.get("RFX_BENCH_EXTEND_TIMEOUT_S", "240")), bail)
        dog.daemon = True
        dog.start()
        try:                                                  # (collective: a failure of any rank is an error on every rank)
            rfx.sharded_assemble_dev(sk.data_ptr(), sc.data_ptr(), ms, prm, gather_below=gather_below)     # untimed warm-up, as below
            sync_all()
            t1 = time.perf_counter()
            text, nc, tr = rfx.sharded_assemble_dev(sk.data_ptr(), sc.data_ptr(), ms, prm, gather_below=gather_below)
            sync_all()
            t_asm = time.perf_counter() - t1
        except reflexiv_amd.RfxError as e:                    # the count stage's line is not lost over the extend stage
            asm_error = str(e)[:400]
        dog.cancel()
        if rank == 0 and asm_error:
            out["contigs"] = {"error": asm_error}
        elif rank == 0:
            lens = sorted((int(h.split("-")[1]) for h in text.split("\n") if h.startswith(">")), reverse=True)
            out["contigs"] = {"driver": "rfx_dev_sharded_assemble: sortByKey as a range shuffle over the ranks while the record set has more than "
                                        + (f"{gather_below}" if gather_below >= 0 else "32 Mi (the default)") + " records, then the one-GPU driver on rank 0",
                              "wall_ms_from_counts": t_asm * 1e3, "wall_ms_reads_to_contigs": t_asm * 1e3 + dt / args.steps * 1e3,
                              "untimed_warmup_runs": 1, "extend_passes": len(tr), "n_contigs": nc, "longest": lens[:3],
                              "total_bases": sum(lens), "sha256_text": __import__("hashlib").sha256(text.encode()).hexdigest()}
        args.no_contigs = True
    if multi and not args.no_contigs and args.sharded_extend and not wide:
        # (the round-2 form over torch.distributed: --exchange-impl torch)
        prm = reflexiv_amd.default_params(k=k, min_cov=args.cover, partitions=max(args.partitions, world))
        ops = rd.HipDevOps(rfx)
        sk, sc = shard["keys"].contiguous(), shard["counts"].contiguous()
        rd.sharded_assemble_dev(ops, sk, sc, prm, force_exchange=args.force_dist)          # untimed warm-up, as below
        sync_all()
        t1 = time.perf_counter()
        tr = []
        text, nc = rd.sharded_assemble_dev(ops, sk, sc, prm, trace=tr, force_exchange=args.force_dist)
        sync_all()
        t_asm = time.perf_counter() - t1
        if rank == 0:
            lens = sorted((int(h.split("-")[1]) for h in text.split("\n") if h.startswith(">")), reverse=True)
            out["contigs"] = {"driver": "range-sharded over the ranks, records resident in HBM (dist.sharded_assemble_dev)",
                              "wall_ms_from_counts": t_asm * 1e3, "wall_ms_reads_to_contigs": t_asm * 1e3 + dt / args.steps * 1e3,
                              "untimed_warmup_runs": 1, "extend_passes": len(tr), "n_contigs": nc, "longest": lens[:3],
                              "total_bases": sum(lens)}
        args.no_contigs = True
    if multi and not args.no_contigs:
        # the filtered list is small: gather it on rank 0, restore ascending k-mer order there
        # and run the extend stage on that one GPU
        torch.cuda.synchronize()
        t_g = time.perf_counter()
        if capi:
            tot_m = rfx.comm_all_reduce([int(shard["counts"].numel())])[0]
            gk = torch.empty(max(1, tot_m) * W, dtype=torch.int64, device=dev) if rank == 0 else shard["keys"][:0]
            gc = torch.empty(max(1, tot_m), dtype=shard["counts"].dtype, device=dev) if rank == 0 else shard["counts"][:0]
            torch.cuda.synchronize()
            got = rfx.gather_shards_dev(shard["keys"].data_ptr(), shard["counts"].data_ptr(), int(shard["counts"].numel()), W,
                                        shard["counts"].element_size(), 0, gk.data_ptr(), gc.data_ptr(), tot_m)
            gk, gc = gk[:got * W], gc[:got]
        else:
            gk, gc = rd.gather_survivors(shard["keys"], shard["counts"], words=W)
        if rank == 0:
            m = int(gc.numel())
            gk = gk.contiguous(); gc = gc.contiguous()
            torch.cuda.synchronize()
            if wide:
                rfx.order_kmers_w_dev(gk.data_ptr(), gc.data_ptr(), m, k)
            else:
                tk = torch.empty_like(gk); tv = torch.empty_like(gc)
                rfx.sort_pairs_dev(gk.data_ptr(), gc.data_ptr(), m, 2 * k, tk.data_ptr(), tv.data_ptr())
            rfx.sync()
            d_keys, d_counts = gk, gc
        t_gather = time.perf_counter() - t_g
    if rank == 0 and not args.no_contigs:
        prm = reflexiv_amd.default_params(k=k, min_cov=args.cover, partitions=args.partitions)
        if wide:
            # the counter's 32-bases-per-word k-mers -> the assembler's 31-bases-per-word layout + its count filter
            # (KmerBinarizer, P/ReflexivDSMain64.java:10772-10836, :473-478), then assemblyFromKmer (:458-826)
            aw = (k - 1) // 31 + 1
            a_k = torch.empty(max(1, m) * aw, dtype=torch.int64, device=dev)
            a_c = torch.empty(max(1, m), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def assemble():
                m2 = rfx.counter_to_asm_dev(d_keys.data_ptr(), d_counts.data_ptr(), m, k, a_k.data_ptr(), a_c.data_ptr(),
                                            args.cover)
                return rfx.assemble_w_dev(a_k.data_ptr(), a_c.data_ptr(), m2, prm)
        else:
            def assemble():
                return rfx.assemble_dev(d_keys.data_ptr(), d_counts.data_ptr(), m, prm)
        # one untimed run first, like the count stage's warm-up steps: the first call of a process loads the
        # extend kernels and grows the record arenas (30 .. 120 ms on a fresh box against 30 ms after)
        assemble()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        text, nc, trace = assemble()
        t_asm = time.perf_counter() - t1
        if multi:
            t_asm += t_gather
        lens = sorted((int(h.split("-")[1]) for h in text.split("\n") if h.startswith(">")), reverse=True)
        out["contigs"] = {"wall_ms_from_counts": t_asm * 1e3, "wall_ms_reads_to_contigs": t_asm * 1e3 + dt / args.steps * 1e3,
                          "untimed_warmup_runs": 1, "extend_passes": len(trace), "n_contigs": nc, "longest": lens[:3],
                          "total_bases": sum(lens), "sha256_text": __import__("hashlib").sha256(text.encode()).hexdigest()}
    if rank == 0 and not args.no_contigs and "contigs" in out and not multi and "error" not in out["contigs"]:
        # contig RC de-duplication (P/ReflexivDSDynamicKmerDedup.java) of the text the path just wrote:
        # the fixed-k path reports every contig on both strands, this reports each once
        rfx.dedup_contig_text(text, 500)                                          # untimed warm-up, as everywhere
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        dtext, dnc, drn = rfx.dedup_contig_text(text, 500)
        t_dd = time.perf_counter() - t1
        dl = sorted((int(h.split("-")[1]) for h in dtext.split("\n") if h.startswith(">")), reverse=True)
        out["contigs"]["dedup"] = {"wall_ms": t_dd * 1e3, "n_contigs": dnc, "contigs_after_each_round": drn, "longest": dl[:3],
                                   "total_bases": sum(dl), "total_bases_before": out["contigs"]["total_bases"]}
    if rank == 0 and not multi and not wide and not args.no_contigs and not args.no_ingest:
        # end-to-end companion of "wall-clock to final contigs": the same reads as ASCII in PINNED host memory through
        # rfx_assemble_reads (upload over PCIe, 2-bit encode, count / filter, extend, text back) -- one call
        nuc = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
        host = torch.empty(n_reads * L, dtype=torch.uint8).pin_memory()
        wv = d_words.view(n_reads, wpr)
        step_r = max(1, (1 << 28) // L)
        for a in range(0, n_reads, step_r):                       # decode the packed reads to ASCII in slices
            b = min(n_reads, a + step_r)
            idx = torch.arange(L, device=dev)
            w = wv[a:b][:, idx // 32]
            code = (w >> (62 - 2 * (idx % 32))) & 3
            host[a * L:b * L].copy_(nuc[code].reshape(-1), non_blocking=True)
            del w, code
        torch.cuda.synchronize()
        roff = (torch.arange(n_reads + 1, dtype=torch.int64) * L).pin_memory().numpy()      # (pinned, like the bases)
        prm_i = reflexiv_amd.default_params(k=k, min_cov=args.cover, partitions=args.partitions)
        rfx.assemble_reads_ptr(host.data_ptr(), n_reads * L, roff, prm_i)            # untimed warm-up, as everywhere
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        text_i, nc_i, trace_i, kept_i = rfx.assemble_reads_ptr(host.data_ptr(), n_reads * L, roff, prm_i)
        t_ing = time.perf_counter() - t1
        out.setdefault("contigs", {})["wall_ms_ascii_to_contigs"] = t_ing * 1e3
        out["contigs"]["ascii_to_contigs"] = {"bytes_over_pcie": n_reads * L, "host_memory": "pinned", "n_contigs": nc_i,
                                              "kmers_kept": kept_i, "same_text_as_resident_path": bool(text_i == text),
                                              "effective_GBps_of_ascii": n_reads * L / t_ing / 1e9}
        del host
    if rank == 0 and not multi and not wide and not args.no_k63 and k == 31:
        # the same reads at k = 63 (BASELINE config 4's k; two-word k-mers): count stage + counts -> contigs, so that the
        # driver's N = 1 run times it too
        out["k63"] = k63_block(args, rfx, torch, reflexiv_amd, d_words, n_reads, wpr, L, dev)
    if rank == 0 and not multi and not wide and not args.no_next_rows and k == 31 and args.gbp == 5.0:
        # the two "next" rows of SURVEY.md 8(f) at the scale a metagenome brings: times and bytes moved
        try:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
            import bench_f2f4
            out["next_rows"] = {"dedup": bench_f2f4.dedup_block(rfx, 50_000), "dyn": bench_f2f4.dyn_block(rfx, 5_000_000)}
        except Exception as e:                                # noqa: BLE001 -- an extra block must not cost the line
            out["next_rows"] = {"error": repr(e)[:300]}
    if rank == 0 and not multi and not wide and not args.no_strong and k == 31 and args.gbp == 5.0:
        # the strong-scaling denominator (VERDICT r03 missing 2): the 50 Gbp set of the 8-GPU configs on this ONE GPU
        del d_words, d_keys, d_counts
        torch.cuda.empty_cache()
        rfx.trim()
        try:
            out["strong_50gbp"] = strong_block(args, rfx, torch, reflexiv_amd, dev)
        except Exception as e:                                # noqa: BLE001 -- an extra block must not cost the line
            out["strong_50gbp"] = {"error": repr(e)[:300]}
    if cpu_record is not None:
        out["cpu_baseline"] = cpu_record
    if rank == 0:
        print(json.dumps(out))
    if multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
