"""Times the k = 65..127 count (three- and four-word k-mers) of config 2's read set (5 Gbp of PE150 from the 4.64 Mbp genome,
-cover 30) synthesised on the device, rfx_dev_count_reads_w, against another build of the package (--ab ROOT: the directory
that holds that build's reflexiv_amd/, for example the parent commit's, whose count at these k is the sort path).  Every
measurement runs in a child process of its own; the children of the two builds alternate, each does --warmup untimed and
--reps timed calls.  Prints one JSON line: per k and build the median, min and max ms, instances, ns per instance, the
workspace high-water (rfx_ctx_workspace_bytes, and hipMemGetInfo's used bytes), the fraction of 8 TB/s that the algorithmic
bytes make (0.25 + 16 W B per instance, 8 W + 8 B per survivor), and the sha256 of the survivors' keys
and counts, which must be the same on both sides; and the medians of the stages' device times (ctx timing: hist1, part1, the
later levels, leaf, sort).  --wide-records 0 sets RFX_WIDE_RECORDS=0 in the children, so that k = 33..63 (--ks 63,47) takes the
same element path at W = 2 instead of its super-k-mer records.

    python tools/w34_bench.py [--ks 81,95,97] [--wide-records 0] [--gbp 5] [--reps 5] [--warmup 2] [--rounds 2] [--ab ROOT]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, a.root)
    import hashlib
    import torch
    import reflexiv_amd
    torch.cuda.set_device(0)
    rfx = reflexiv_amd.Reflexiv(0)
    L, k = 150, a.k
    W = k // 32 + 1
    n = int(a.gbp * 1e9) // L
    wpr = (L + 31) // 32
    dg = torch.empty((a.genome + 31) // 32, dtype=torch.int64, device="cuda")
    dw = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rfx.synth_genome_dev(a.seed, a.genome, dg.data_ptr())
    rfx.synth_reads_dev(a.seed, dg.data_ptr(), a.genome, 0, n, L, wpr, dw.data_ptr())
    rfx.sync()
    del dg
    cap = 64 << 20
    dk = torch.empty(cap * W, dtype=torch.int64, device="cuda")
    dc = torch.empty(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    free0, total = torch.cuda.mem_get_info()
    times, stages, used_hw, ws_hw, r = [], [], 0, 0, None
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = rfx.count_reads_w_dev(dw.data_ptr(), n, wpr, L, k, dk.data_ptr(), dc.data_ptr(), cap, a.cover)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        free, _ = torch.cuda.mem_get_info()
        used_hw = max(used_hw, free0 - free)
        ws_hw = max(ws_hw, rfx.workspace_bytes())
        if rep >= a.warmup:
            times.append(dt)
            t = rfx.count_timing()
            stages.append({"hist1": t.get("hist1", (0, 0))[0], "part1": t.get("part1", (0, 0))[0],
                           "levels": sum(v[0] for nm, v in t.items()
                                         if nm.startswith(("hist", "part")) and nm not in ("hist1", "part1")),
                           "leaf": t.get("leaf", (0, 0))[0], "sort": t.get("sort", (0, 0))[0]})
    m, nd, inst = r
    h = hashlib.sha256()
    h.update(dk[:W * m].cpu().numpy().tobytes())
    h.update(dc[:m].cpu().numpy().tobytes())
    t = rfx.count_timing()
    rfx.close()
    print(json.dumps({"times": times, "stages": stages, "instances": inst, "distinct": nd, "kept": m, "sha256": h.hexdigest(),
                      "workspace_bytes": ws_hw, "mem_used_bytes": used_hw, "leaf": "leaf" in t, "sort_path": "count_w" in t}))


def summarise(k, runs):
    W = k // 32 + 1
    ts = sorted(t for r in runs for t in r["times"])
    r0 = runs[-1]
    med = ts[len(ts) // 2]
    algo = (0.25 + 16 * W) * r0["instances"] + (8 * W + 8) * r0["kept"]
    st = [x for r in runs for x in r["stages"]]
    stage_ms = {nm: round(sorted(x[nm] for x in st)[len(st) // 2], 2) for nm in st[0]}
    return {"ms_median": round(med, 2), "ms_min": round(ts[0], 2), "ms_max": round(ts[-1], 2), "reps": len(ts),
            "instances": r0["instances"], "distinct": r0["distinct"], "kept": r0["kept"],
            "ns_per_instance": round(med * 1e6 / max(1, r0["instances"]), 4),
            "workspace_gib": round(max(r["workspace_bytes"] for r in runs) / 2**30, 2),
            "mem_used_gib": round(max(r["mem_used_bytes"] for r in runs) / 2**30, 2),
            "frac_of_8TBps": round(algo / (med * 1e-3) / 8e12, 4), "sha256": r0["sha256"], "leaf": r0["leaf"],
            "sort_path": r0["sort_path"], "stage_ms_median": stage_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="81,95,97")
    ap.add_argument("--k", type=int, default=95)
    ap.add_argument("--gbp", type=float, default=5.0)
    ap.add_argument("--genome", type=int, default=4_640_000)
    ap.add_argument("--cover", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--wide-records", choices=["0", "1"], default=None, help="RFX_WIDE_RECORDS of the children (k = 33..63)")
    ap.add_argument("--ab", default=None, help="the other build's root (holds reflexiv_amd/)")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sides = {"this": HERE}
    if a.ab:
        sides["other"] = os.path.abspath(a.ab)
    out = {"gbp": a.gbp, "cover": a.cover, "wide_records": a.wide_records, "reps_per_child": a.reps, "warmup": a.warmup, "rounds": a.rounds}
    for k in [int(x) for x in a.ks.split(",")]:
        runs = {s: [] for s in sides}
        for rnd in range(a.rounds):
            for s, root in (sides.items() if rnd % 2 == 0 else reversed(list(sides.items()))):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--k", str(k), "--gbp", str(a.gbp),
                       "--genome", str(a.genome), "--cover", str(a.cover), "--reps", str(a.reps), "--warmup", str(a.warmup),
                       "--seed", str(a.seed)]
                env = dict(os.environ, **({"RFX_WIDE_RECORDS": a.wide_records} if a.wide_records else {}))
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
                if p.returncode != 0:
                    out[f"k{k}_{s}_error"] = (p.stdout + p.stderr)[-1500:]
                    print(json.dumps(out), flush=True)
                    sys.exit(1)
                runs[s].append(json.loads(p.stdout.strip().splitlines()[-1]))
        res = {s: summarise(k, rs) for s, rs in runs.items()}
        if "other" in res:
            res["same_survivors"] = res["this"]["sha256"] == res["other"]["sha256"]
            res["speedup"] = round(res["other"]["ms_median"] / res["this"]["ms_median"], 3)
        out[f"k{k}"] = res
        print(json.dumps({f"k{k}": res}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
