#!/usr/bin/env python3
"""Minimum spanning tree and closest row on the device (uvaia_gpu_db_near_*, uvaia_gpu_db_mst, kernels_pairs.inc) on the GPU box.  The
numbers are recorded; what is checked is only that the forms agree with each other (the rounds driven from here build the edges db_mst
hands back, the tree has refs - 1 edges).
  (a) kernel against kernel  generator genomes (host/synth.c, SARS-CoV-2 length) resident in one engine; over rows [0, --rows) x columns
                             [0, --refs) and every reference a component of its own (nothing skipped): device time of the snp near kernel
                             with the floor off and on (uvaia_gpu_near_ms), of the snp link kernel with the floor off and on
                             (uvaia_gpu_link_ms) and of pairs_snp_kernel<32> (uvaia_gpu_pairs_ms), then of the near mode and the link mode of
                             pairs_counts_kernel under the uvaia metric; one process, the kernels alternate within a round; one warming
                             round, --rounds counted ones, median and min-max
  (b) the tree               uvaia_gpu_db_mst of the --refs rows: wall time and device time; the same rounds driven from here for the device
                             time and the tile pairs walked and skipped of every round; one dense pass of the same rows (uvaia_gpu_db_pairs
                             in bands) next to it
  (c) whole commands         `uvaiadist --packed --mst` and `--nearest` against the plain square table of the same file, to /dev/null;
                             one warming round and --command-rounds counted ones, the three forms alternating
Writes profiles/pair_mst.json and prints it.
Usage: python tools/pair_mst_bench.py [--refs 20000] [--rows 4096] [--dir /tmp/pair_mst]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from uvaia_amd import capi, hostlib  # noqa: E402

NCHAR = 29903
NONE = np.uint64(capi.NEAR_NONE)


def spread(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "all_ms": [round(x, 3) for x in v]}


def open_engine(a, n):
    import oracle_lib as O
    gen = hostlib.Synth()
    root = bytes(b"ACGT"[s & 3] for s in range(NCHAR))
    eng = capi.Engine.from_query(O.Query([root], ["q"]), nbest=1, max_pool=64, device=a.device)
    eng.db_reserve(n)
    for first in range(0, n, 4096):
        rows, non_n = gen.generate(first, min(4096, n - first))
        eng.db_append_block(rows, non_n)
    return eng


def kernels(a, eng, doc):
    rect = dict(rows=(0, a.rows), cols=(0, a.refs))
    out = np.zeros((a.rows, a.refs), dtype=np.int32)

    def near(metric, floor):
        eng.db_near_begin(metric=metric, min_compared=floor)
        eng.near_ms(reset=True)
        stats = eng.db_near(**rect)
        return eng.near_ms(), stats

    def link(metric, floor):
        eng.db_link_begin(2, metric=metric, min_compared=floor)
        eng.link_ms(reset=True)
        eng.db_link(**rect)
        return eng.link_ms(), None

    def dense():
        eng.pairs_ms(reset=True)
        eng.db_pairs(out=out, **rect)
        return eng.pairs_ms()["dense"], None
    runs = {"near_snp_floor_off": lambda: near(capi.DIST_SNP, 0), "link_snp_floor_off": lambda: link(capi.DIST_SNP, 0), "pairs_snp_kernel_32": dense,
            "near_snp_floor_on": lambda: near(capi.DIST_SNP, 1), "link_snp_floor_on": lambda: link(capi.DIST_SNP, 1),
            "near_uvaia": lambda: near(capi.DIST_UVAIA, 0), "link_uvaia": lambda: link(capi.DIST_UVAIA, 0)}
    ms = {k: [] for k in runs}
    tiles = {}
    for r in range(a.rounds + 1):
        for key, run in runs.items():                   # the kernels alternate within a round
            t, stats = run()
            if r:
                ms[key].append(t)
            if stats:
                tiles[key] = {"walked": stats[0], "skipped": stats[1]}
    res = {k: dict(spread(v), rows=a.rows, cols=a.refs, **({"tile_pairs": tiles[k]} if k in tiles else {})) for k, v in ms.items()}
    s = {}
    for num, den in (("near_snp_floor_off", "link_snp_floor_off"), ("near_snp_floor_off", "pairs_snp_kernel_32"), ("near_snp_floor_on", "link_snp_floor_on"), ("near_uvaia", "link_uvaia")):
        s["%s_over_%s" % (num, den)] = round(res[num]["median_ms"] / res[den]["median_ms"], 3)
    doc["kernel_against_kernel"] = dict(res, ratios_of_medians=s)


def one_round(eng, n, comp, edges):
    """a round of uvaia_gpu_db_mst's protocol driven from here: (device ms, walked, skipped, edges added, the new components)"""
    import pair_link as K
    eng.db_near_components(comp)
    eng.near_ms(reset=True)
    walked, skipped = eng.db_near()
    ms = eng.near_ms()
    best = eng.db_near_fetch()
    x = np.flatnonzero(best != NONE)
    d, y = (best[x] >> np.uint64(32)).astype(np.int64), (best[x] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    lo, hi = np.minimum(x, y), np.maximum(x, y)
    cx = (np.arange(n) if comp is None else comp)[x]
    order = np.lexsort((hi, lo, d, cx))
    first = order[np.concatenate([[True], cx[order][1:] != cx[order][:-1]])] if len(order) else order
    chosen = sorted(set(zip(lo[first].tolist(), hi[first].tolist(), d[first].tolist())))      # an edge chosen from both sides goes in once
    edges.extend(chosen)
    return ms, walked, skipped, len(chosen), K.components(n, [(p, q) for p, q, _d in edges])


def tree(a, eng, doc):
    n = a.refs
    res = {"refs": n}
    wall, dev, rows_ms = [], [], []
    for r in range(a.rounds + 1):
        eng.near_ms(reset=True)
        eng.pairs_ms(reset=True)
        eng.near_tiles(reset=True)
        t0 = time.perf_counter()
        records, rounds = eng.db_mst()
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(eng.near_ms())
            rows_ms.append(eng.pairs_ms()["rows"])
    walked, skipped = eng.near_tiles()
    res["db_mst"] = {"wall": spread(wall), "near_kernels": spread(dev), "row_operands": spread(rows_ms), "rounds": rounds, "edges": int(len(records)),
                     "weight": int(records["dist"].sum()), "tile_pairs_walked": walked, "tile_pairs_skipped": skipped}
    # the same rounds from here, for the figures of every round
    eng.db_near_begin()
    comp, edges, per_round = None, [], []
    while len(edges) < n - 1 and len(per_round) < 64:
        ms, walked, skipped, added, comp = one_round(eng, n, comp, edges)
        per_round.append({"near_kernel_ms": round(ms, 3), "tile_pairs_walked": walked, "tile_pairs_skipped": skipped, "edges_added": added, "components_left": int(len(np.unique(comp)))})
        if not added:
            break
    res["rounds_driven_from_python"] = per_round
    mine = sorted(edges, key=lambda e: (e[2], e[0], e[1]))
    res["the_rounds_build_the_edges_of_db_mst"] = bool(mine == [(int(p), int(q), int(d)) for p, q, d in zip(records["a"], records["b"], records["dist"])])
    # one dense pass of the same rows, in bands
    out = np.zeros((a.rows, n), dtype=np.int32)
    dense = []
    for r in range(a.rounds + 1):
        eng.pairs_ms(reset=True)
        for first in range(0, n, a.rows):
            eng.db_pairs(rows=(first, min(a.rows, n - first)), cols=(0, n), out=out)
        if r:
            dense.append(eng.pairs_ms()["dense"])
    res["dense_pass_pairs_snp_kernel_32"] = spread(dense)
    res["tree_over_one_dense_pass"] = round(res["db_mst"]["near_kernels"]["median_ms"] / res["dense_pass_pairs_snp_kernel_32"]["median_ms"], 3)
    doc["tree"] = res


def whole_command(a, doc):
    os.makedirs(a.dir, exist_ok=True)
    gen = hostlib.Synth()
    fa, db = os.path.join(a.dir, "refs.fa"), os.path.join(a.dir, "refs.uvdb")
    with open(fa, "wb") as fh:
        for first in range(0, a.refs, 2048):
            rows, _ = gen.generate(first, min(2048, a.refs - first))
            for i in range(rows.shape[0]):
                fh.write(b">ref_%d\n" % (first + i) + rows[i].tobytes() + b"\n")
    subprocess.check_call([os.path.join(ROOT, "bin", "uvaiapack"), "-A", "1", "-o", db, fa], stderr=subprocess.DEVNULL)
    os.remove(fa)
    res = {"mst": [], "nearest": [], "table": []}
    for rnd in range(a.command_rounds + 1):             # one warming round, then the counted ones; the three forms alternate
        for key, form in (("table", []), ("mst", ["--mst"]), ("nearest", ["--nearest"])):
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(ROOT, "bin", "uvaiadist"), "-o", "/dev/null"] + form + ["--packed", db], stderr=subprocess.PIPE, check=True, timeout=300)
            rep = json.loads(re.search(rb"dist report: (\{.*\})", r.stderr).group(1))
            rep["wall_s"] = round(time.perf_counter() - t0, 2)
            if rnd:
                res[key].append(rep)
    res["median_wall_s"] = {k: statistics.median(x["wall_s"] for x in v) for k, v in res.items()}
    doc["whole_command_to_dev_null"] = res
    os.remove(db)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--command-rounds", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dir", default="/tmp/pair_mst")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_mst.json"))
    a = ap.parse_args()
    doc = {"nchar": NCHAR, "refs": a.refs, "rounds": a.rounds,
           "instructions_per_pair_word": {"pairs_snp_kernel_32": 4, "near_snp_floor_off": 4, "near_snp_floor_on": 6, "link_snp_floor_off": 4, "link_snp_floor_on": 6, "pairs_counts_kernel": 17},
           "not_measured": ["a cold cache", "100 000 rows", "dense near-identical sets beyond the 4 160-row test"], "failed": []}
    eng = open_engine(a, a.refs)
    steps = (("kernels", lambda: kernels(a, eng, doc)), ("tree", lambda: tree(a, eng, doc)), ("close", eng.close), ("whole_command", lambda: whole_command(a, doc)))
    for name, f in steps:
        try:
            f()
            failed = None
        except Exception as e:       # what could not be run is named and nothing more is started; what was measured is still written
            failed = "%s and what follows it: %s" % (name, e)
            doc["failed"].append(failed)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        if failed:
            break
    print(json.dumps(doc))
    if doc["failed"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
