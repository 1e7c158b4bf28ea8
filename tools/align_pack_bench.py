#!/usr/bin/env python3
"""Raw genomes to a packed database on the GPU box, whole commands: (a) `uvaialign -o` followed by `uvaiapack` against (b) `uvaialign --packed`,
on unaligned sequences of SARS-CoV-2 length from the generator the aligner benchmark uses (bench.py config[4]).  The two ways alternate, three
runs each after a warm-up of both; the files must be identical.  The device time of the alignment kernels and of the three kernels of the
pack stage (census, gather, exception runs; HIP events) is what `uvaialign --packed` reports on its last line.  Writes one JSON document;
every number carries the command that produced it.

Usage: python tools/align_pack_bench.py [--queries 10000] [--pool 4096] [--dir /tmp/align_pack] [--out profiles/align_pack.json]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from uvaia_amd import hostlib  # noqa: E402

ALIGN, PACK = os.path.join(ROOT, "bin", "uvaialign"), os.path.join(ROOT, "bin", "uvaiapack")


def run(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    err = r.stderr.decode(errors="replace")
    if r.returncode:
        sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), err[-3000:]))
        sys.exit(1)
    return {"command": " ".join(os.path.relpath(c, ROOT) if c.startswith(ROOT) else c for c in cmd), "wall_s": round(dt, 3),
            "progress_lines": [l for l in err.splitlines() if "Total elapsed" in l or "Packed" in l or "Device time" in l]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--dir", default="/tmp/align_pack")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_pack.json"))
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    gen = hostlib.Synth(29903, seed=20241008, preset=1)
    ref = np.array(gen.generate(7, 1)[0][0], dtype=np.uint8)
    ref[~np.isin(ref, np.frombuffer(b"ACGT", dtype=np.uint8))] = ord("A")
    gen = hostlib.Synth(29903, seed=20241008, preset=0)
    rng = np.random.default_rng(20241008)
    ref_fa, q_fa = os.path.join(a.dir, "ref.fa"), os.path.join(a.dir, "raw.fa")
    with open(ref_fa, "wb") as fh:
        fh.write(b">reference\n" + ref.tobytes() + b"\n")
    n = 0
    with open(q_fa, "wb") as fh:
        for first in range(0, a.queries, 2048):
            rows, _ = gen.generate(bench.QUERY_INDEX0 + first, min(2048, a.queries - first))
            for s in bench.unaligned_from_rows(np.asarray(rows, dtype=np.uint8), rng):
                fh.write(b">q_%d\n" % n + s + b"\n")
                n += 1
    common = ["-r", ref_fa, q_fa, "-a", "1.0", "-p", str(a.pool)]
    text, db_a, db_b = os.path.join(a.dir, "aligned"), os.path.join(a.dir, "a.uvdb"), os.path.join(a.dir, "b.uvdb")

    def way_a():
        one = run([ALIGN] + common + ["-o", text])
        two = run([PACK, "-o", db_a, text + ".aln.xz"])
        return {"uvaialign": one, "uvaiapack": two, "wall_s": round(one["wall_s"] + two["wall_s"], 3)}

    def way_b():
        return run([ALIGN] + common + ["--packed", db_b])

    way_a(); way_b()                                                   # page cache, code objects, device warm
    runs_a, runs_b = [], []
    for _ in range(3):
        runs_a.append(way_a())
        runs_b.append(way_b())
    same = open(db_a, "rb").read() == open(db_b, "rb").read()
    med = lambda v: sorted(x["wall_s"] for x in v)[1]
    device = []
    for r in runs_b:
        m = re.search(r"alignment ([\d.]+) ms; census ([\d.]+) ms, gather ([\d.]+) ms, exception runs ([\d.]+) ms", " ".join(r["progress_lines"]))
        if m:
            device.append(dict(zip(("wfa_align_kernel_passes_ms", "rows_census_kernel_ms", "rows_gather_kernel_ms", "rows_fill_exceptions_kernel_ms"), (float(x) for x in m.groups()))))
    doc = {"sequences": n, "nchar": 29903, "pool": a.pool, "raw_fasta_bytes": os.path.getsize(q_fa), "uvdb_bytes": os.path.getsize(db_b), "aligned_xz_bytes": os.path.getsize(text + ".aln.xz"),
           "same_file": bool(same),
           "a_uvaialign_then_uvaiapack": {"median_wall_s": med(runs_a), "runs": runs_a},
           "b_uvaialign_packed": {"median_wall_s": med(runs_b), "runs": runs_b},
           "b_over_a": round(med(runs_b) / med(runs_a), 4),
           "device_time_of_b": device,
           "note": "wall clock of whole commands on one box, (a) and (b) alternating after one warm-up of each; device times from HIP events around the kernels, "
                   "summed over the pools of one run (the gather figure is the gather alone, pack_refs_kernel follows it as in uvaia_gpu_db_append)"}
    if device:
        d = device[len(device) // 2]
        three = d["rows_census_kernel_ms"] + d["rows_gather_kernel_ms"] + d["rows_fill_exceptions_kernel_ms"]
        doc["pack_stage_kernels_over_alignment_kernels"] = round(three / max(d["wfa_align_kernel_passes_ms"], 1e-9), 5)
        doc["pack_stage_kernels_share_of_command"] = round(three / 1000. / med(runs_b), 5)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    if not same:
        sys.exit("the two ways wrote different files")


if __name__ == "__main__":
    main()
