"""uvaiaclust: the default residency mode (every pushed row kept) against keep medoids (uvaia_clust_keep_medoids) on the synthetic
workload of tools/cluster_bench.py: 100 000 family rows, d = 3, 64 queues, pushes of 256 rows.  Five runs of each mode, alternating: per-phase
kernel milliseconds, wall time and peak row bytes per run, medians, and the max - min spread of each mode's kernel total.  Writes
profiles/cluster_keep.json (--out).  A library without the mode (a build of an earlier commit) gives the default mode's numbers only; run there
with --out profiles/cluster_keep_parent.json and name that file here with --parent: the default mode of the two builds is then compared
within the parent's spread, and the ratio keep medoids / default of this build is recorded."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cluster_lib as CL  # noqa: E402
from uvaia_amd import cluster  # noqa: E402


def one(ref, seqs, queues, dist, n_queues, push, keep):
    t0 = time.perf_counter()
    with cluster.Clusterer(ref, dist=dist, trim=0, n_score=1, n_queues=n_queues) as c:
        if keep:
            c.keep_medoids(0)
        for a in range(0, len(seqs), push):
            c.push(seqs[a:a + push], queues[a:a + push])
        c.finish()
        wall = time.perf_counter() - t0
        st = c.stats()
        res = c.result()
        mem = c.memory() if hasattr(c, "memory") else {"peak_row_bytes": None}
    return {"prep_ms": round(st["prep_ms"], 3), "queue_ms": round(st["queue_ms"], 3), "merge_ms": round(st["merge_ms"], 3),
            "kernel_ms": round(st["prep_ms"] + st["queue_ms"] + st["merge_ms"], 3), "wall_s": round(wall, 4),
            "peak_row_bytes": mem["peak_row_bytes"]}, (res.clusters(), res.scores.tolist())


def summary(runs):
    k = [r["kernel_ms"] for r in runs]
    return {"runs": runs, "median_kernel_ms": round(statistics.median(k), 3), "spread_kernel_ms": round(max(k) - min(k), 3),
            "median_prep_ms": round(statistics.median(r["prep_ms"] for r in runs), 3), "median_queue_ms": round(statistics.median(r["queue_ms"] for r in runs), 3),
            "median_merge_ms": round(statistics.median(r["merge_ms"] for r in runs), 3), "median_wall_s": round(statistics.median(r["wall_s"] for r in runs), 4),
            "peak_row_bytes": runs[0]["peak_row_bytes"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_keep.json"))
    ap.add_argument("--parent", default=None, help="the file this tool wrote on a build of the parent commit")
    ap.add_argument("--synthetic", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    n_queues, dist, push = 64, 3, 256
    seqs = CL.families(a.synthetic, a.synthetic // 13, 20261017)
    ref = CL.rs_reference(seqs[:1024])
    queues = CL.round_robin([len(seqs)], n_queues)
    modes = ["keep_all"] + (["keep_medoids"] if hasattr(cluster.Clusterer, "keep_medoids") else [])
    one(ref, seqs[:2048], queues[:2048], dist, n_queues, push, False)               # warm-up: module load, first allocations
    runs, answers = {m: [] for m in modes}, []
    for _ in range(a.runs):
        for m in modes:
            r, ans = one(ref, seqs, queues, dist, n_queues, push, m == "keep_medoids")
            runs[m].append(r)
            answers.append(ans)
            print(json.dumps({"mode": m, **r}), flush=True)
    out = {"workload": "synthetic_families_d3", "n": len(seqs), "nchar": len(ref), "dist": dist, "queues": n_queues, "push": push, "clusters": len(answers[0][0]),
           "identical_results": all(x == answers[0] for x in answers)}
    for m in modes:
        out[m] = summary(runs[m])
    if "keep_medoids" in out:
        out["keep_medoids_over_keep_all_kernel"] = round(out["keep_medoids"]["median_kernel_ms"] / out["keep_all"]["median_kernel_ms"], 4)
        out["keep_medoids_over_keep_all_wall"] = round(out["keep_medoids"]["median_wall_s"] / out["keep_all"]["median_wall_s"], 4)
    if a.parent:
        par = json.load(open(a.parent))["keep_all"]
        diff = abs(out["keep_all"]["median_kernel_ms"] - par["median_kernel_ms"])
        out["parent_keep_all"] = par
        out["keep_all_against_parent"] = {"median_difference_ms": round(diff, 3), "parent_spread_ms": par["spread_kernel_ms"], "within_parent_spread": diff <= par["spread_kernel_ms"]}
        if "keep_medoids" in out:
            slower = out["keep_medoids"]["median_kernel_ms"] - out["keep_all"]["median_kernel_ms"]
            out["keep_medoids_slower_than_parent_spread"] = slower > par["spread_kernel_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, dict)}), flush=True)
    if not out["identical_results"]:
        sys.exit("the modes or the runs differ in their clusters")


if __name__ == "__main__":
    main()
