#!/usr/bin/env python3
"""What keeping the insertion runs costs on the GPU box: the workload of `bench.py --align-only` (BASELINE config[4]: 10 000 unaligned
generator genomes against one reference of 29 903 sites, Poisson-2 insertions of 1-12 characters in each) through uvaia_align_run with the
option off and on, alternating in one process on one resident pool, and the whole command `uvaialign --packed` with and without
`--insertions`, alternating, with a warm page cache.  The rows, scores and cells of the two kernels are compared, and the table of the
command with the records of the library.  Prints one JSON line; profiles/align_insertions.json holds such a line as "run", next to "tool",
"where" and "note", which were written by hand.
Usage: python tools/align_insertions_bench.py [--queries 10000] [--rounds 5] [--cli-rounds 3] [--dir /tmp/align_insertions]"""
import argparse
import filecmp
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
import bench  # noqa: E402
from uvaia_amd import align, hostlib  # noqa: E402

NCHAR, SEED = 29903, 20241008


def workload(queries):
    """reference and queries as bench.align_workload makes them"""
    gen = hostlib.Synth(NCHAR, seed=SEED, preset=1)
    ref = np.array(gen.generate(7, 1)[0][0], dtype=np.uint8)
    ref[~np.isin(ref, np.frombuffer(b"ACGT", dtype=np.uint8))] = ord("A")
    gen = hostlib.Synth(NCHAR, seed=SEED, preset=0)
    rng = np.random.default_rng(SEED)
    seqs = []
    for first in range(0, queries, 2048):
        rows, _ = gen.generate(bench.QUERY_INDEX0 + first, min(2048, queries - first))
        seqs += bench.unaligned_from_rows(np.asarray(rows, dtype=np.uint8), rng)
    return ref.tobytes(), seqs


def spread(xs):
    return {"runs": [round(x, 3) for x in xs], "median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def library(ref, seqs, rounds):
    out = {}
    with align.Aligner(ref) as al:
        al.load(seqs)
        al.run()                                                # warm-up: the workspace
        ms = {"off": [], "on": []}
        answer = {}
        for rnd in range(rounds + 1):                           # round 0 warms both kernels and is not counted
            for mode in ("off", "on"):
                al.set_insertions(mode == "on")
                al.run()
                st = al.stats()
                if rnd:
                    ms[mode].append(st["kernel_ms"])
                else:
                    score, rows = al.fetch()
                    answer[mode] = (score.copy(), rows.copy(), st["cells"], st["passes"])
        table = al.insertions()
    off, on = spread(ms["off"]), spread(ms["on"])
    width = off["max"] - off["min"]
    out["kernel_ms_per_pool"] = {"off": off, "on": on, "on_minus_off_median": round(on["median"] - off["median"], 3), "off_spread": round(width, 3),
                                 "on_within_off_spread": on["median"] <= off["median"] + width}
    out["same_rows_scores_cells_passes"] = bool(np.array_equal(answer["off"][0], answer["on"][0]) and np.array_equal(answer["off"][1], answer["on"][1]) and answer["off"][2:] == answer["on"][2:])
    out["passes"] = answer["on"][3]
    out["records"] = len(table)
    out["inserted_bases"] = sum(len(b) for *_, b in table)
    out["sequences_with_insertions"] = len({q for q, *_ in table})
    return out, table


def command(d, ref, seqs, table, rounds):
    ref_fa, fa = os.path.join(d, "ref.fa"), os.path.join(d, "queries.fa")
    with open(ref_fa, "wb") as fh:
        fh.write(b">reference\n" + ref + b"\n")
    with open(fa, "wb") as fh:
        for i, s in enumerate(seqs):
            fh.write(b">q_%d\n" % i + s + b"\n")
    exe = os.path.join(ROOT, "bin", "uvaialign")
    cmds = {"plain": [exe, "-r", ref_fa, "-a", "1.0", "--packed", os.path.join(d, "plain.uvdb"), fa],
            "insertions": [exe, "-r", ref_fa, "-a", "1.0", "--packed", os.path.join(d, "ins.uvdb"), "--insertions", os.path.join(d, "ins.csv"), fa]}
    wall, dev = {k: [] for k in cmds}, {k: [] for k in cmds}
    for rnd in range(rounds + 1):                               # round 0 warms the page cache and is not counted
        for k, c in cmds.items():
            t0 = time.perf_counter()
            r = subprocess.run(c, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
            w = time.perf_counter() - t0
            err = r.stderr.decode(errors="replace")
            if r.returncode:
                sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(c), err[-3000:]))
                sys.exit(1)
            sys.stderr.write("command round %d %s: %.3f s\n" % (rnd, k, w))
            sys.stderr.flush()
            if rnd:
                wall[k].append(w)
                dev[k].append(float(re.search(r"Device time: alignment ([0-9.]+) ms", err).group(1)))
    want = b"sequence,ref_pos,length,bases\n" + b"".join(b"q_%d,%d,%d,%s\n" % (q, r, len(b), b) for q, r, _, b in table)
    p = spread(wall["plain"])
    out = {"command": "uvaialign -r ref.fa -a 1.0 --packed out.uvdb [--insertions out.csv] queries.fa", "wall_s": {"plain": p, "insertions": spread(wall["insertions"])},
           "align_ms": {k: spread(v) for k, v in dev.items()}, "same_database": filecmp.cmp(os.path.join(d, "plain.uvdb"), os.path.join(d, "ins.uvdb"), shallow=False),
           "table_is_the_librarys": open(os.path.join(d, "ins.csv"), "rb").read() == want, "table_bytes": len(want)}
    out["insertions_within_plain_spread"] = out["wall_s"]["insertions"]["median"] <= p["median"] + (p["max"] - p["min"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cli-rounds", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/align_insertions")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    ref, seqs = workload(a.queries)
    result = {"queries": len(seqs), "nchar": NCHAR, "rounds": a.rounds, "cli_rounds": a.cli_rounds, "cold_cache": "not measured"}
    result["library"], table = library(ref, seqs, a.rounds)
    if a.cli_rounds > 0:
        result["command"] = command(a.dir, ref, seqs, table, a.cli_rounds)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
