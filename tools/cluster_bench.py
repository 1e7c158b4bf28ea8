"""uvaiaclust: GPU kernel time per phase against the CPU restatement (tests/cluster_restatement.c, OpenMP over the queues) on the
bench workloads: the bundled alignment at d = 1, 10, 300 with 64 queues, and 100 000 synthetic family sequences at d = 3.
Prints one JSON line per workload and, with --out, writes them all to a file.  Both sides get the same rows and queues and must
give the same clusters."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cluster_lib as CL  # noqa: E402
import fixtures as F  # noqa: E402
from uvaia_amd import cluster  # noqa: E402


def run(name, ref, seqs, dist, n_queues, trim=0, n_score=1, reps=3):
    queues = CL.round_robin([len(seqs)], n_queues)
    d, t, s = CL.clamp(len(ref), dist, trim, n_score)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        with cluster.Clusterer(ref, dist=d, trim=t, n_score=s, n_queues=n_queues) as c:
            for a in range(0, len(seqs), 4 * n_queues):
                c.push(seqs[a:a + 4 * n_queues], queues[a:a + 4 * n_queues])
            c.finish()
            wall = time.perf_counter() - t0
            st = c.stats()
            res = c.result()
        tot = st["prep_ms"] + st["queue_ms"] + st["merge_ms"]
        if best is None or tot < best[0]:
            best = (tot, st, wall, res)
    tot, st, wall, res = best
    t0 = time.perf_counter()
    want, want_scores = CL.rs_cluster(ref, seqs, queues, d, t, s, n_queues)
    cpu = time.perf_counter() - t0
    same = res.clusters() == want and res.scores.tolist() == want_scores.tolist()
    rows_bytes = len(seqs) * len(ref)
    line = {"workload": name, "n": len(seqs), "nchar": len(ref), "dist": d, "queues": n_queues, "trim": t, "snps": s, "clusters": len(want),
            "gpu_prep_ms": round(st["prep_ms"], 3), "gpu_queue_ms": round(st["queue_ms"], 3), "gpu_merge_ms": round(st["merge_ms"], 3),
            "gpu_kernel_ms": round(tot, 3), "gpu_wall_s": round(wall, 3), "cpu_restatement_s": round(cpu, 3), "cpu_threads": CL.restatement().rs_threads(),
            "speedup_kernels": round(cpu * 1e3 / tot, 1) if tot else None, "speedup_wall": round(cpu / wall, 1),
            "prep_gbps_algorithmic": round(rows_bytes / (st["prep_ms"] * 1e-3) / 1e9, 1) if st["prep_ms"] else None,
            "per_queue_step_us": round(st["queue_ms"] * 1e3 / max(1, (len(seqs) + n_queues - 1) // n_queues), 3), "identical": same}
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--synthetic", type=int, default=100000)
    a = ap.parse_args()
    names, seqs = F.load_bundled()
    ref = CL.rs_reference(seqs[:1024])
    lines = [run("bundled_d%d" % d, ref, seqs, d, 64) for d in (1, 10, 300)]
    fam = CL.families(a.synthetic, a.synthetic // 13, 20261017)
    lines.append(run("synthetic_families_d3", CL.rs_reference(fam[:1024]), fam, 3, 64, reps=2))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(lines, fh, indent=1)
    if not all(l["identical"] for l in lines):
        sys.exit("GPU and restatement differ")


if __name__ == "__main__":
    main()
