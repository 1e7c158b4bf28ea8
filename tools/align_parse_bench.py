#!/usr/bin/env python3
"""`uvaialign --device-parse` against `uvaialign` and against the parent commit's `uvaialign` on the GPU box: the generator genomes of
tools/align_cli_bench.py (the BASELINE config[4] workload of bench.py as unaligned FASTA) with one line per sequence, wrapped at 60 and as
.gz, written to a packed database (--packed) and to an xz file (-o).  One warming round, then counted rounds that alternate the three
commands on the same file, with a warm page cache.  The outputs of the three commands are compared.  Prints one JSON line;
profiles/align_device_parse.json holds such a line as "run", next to "tool", "parent", "where" and "note", which were written by hand.
Usage: python tools/align_parse_bench.py --parent-bin <parent checkout>/bin [--queries 10000] [--rounds 3] [--dir /tmp/align_parse] [--outputs packed,xz]"""
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
from uvaia_amd import hostlib  # noqa: E402


def write_inputs(d, queries):
    """reference and queries as tools/align_cli_bench.py writes them; the queries on one line, wrapped at 60, and the one-line file as .gz"""
    gen = hostlib.Synth(29903, seed=20241008, preset=1)
    ref = np.array(gen.generate(7, 1)[0][0], dtype=np.uint8)
    ref[~np.isin(ref, np.frombuffer(b"ACGT", dtype=np.uint8))] = ord("A")
    gen = hostlib.Synth(29903, seed=20241008, preset=0)
    rng = np.random.default_rng(20241008)
    ref_fa, plain, wrap60 = os.path.join(d, "ref.fa"), os.path.join(d, "queries.fa"), os.path.join(d, "queries60.fa")
    with open(ref_fa, "wb") as fh:
        fh.write(b">reference\n" + ref.tobytes() + b"\n")
    n = 0
    with open(plain, "wb") as one, open(wrap60, "wb") as wrapped:
        for first in range(0, queries, 2048):
            rows, _ = gen.generate(bench.QUERY_INDEX0 + first, min(2048, queries - first))
            for s in bench.unaligned_from_rows(np.asarray(rows, dtype=np.uint8), rng):
                one.write(b">q_%d\n" % n + s + b"\n")
                wrapped.write(b">q_%d\n" % n + b"".join(s[a:a + 60] + b"\n" for a in range(0, len(s), 60)))
                n += 1
    subprocess.check_call("gzip -1 -c %s > %s.gz" % (plain, plain), shell=True)
    return ref_fa, {"plain": plain, "wrap60": wrap60, "gz": plain + ".gz"}, n


def run(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    err = r.stderr.decode(errors="replace")
    if r.returncode:
        sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), err[-3000:]))
        sys.exit(1)
    dev = re.search(r"device parse: (\{.*\})", err)
    return wall, json.loads(dev.group(1)) if dev else None


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", required=True, help="bin/ of a built checkout of the parent commit")
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/align_parse")
    ap.add_argument("--forms", default="plain,wrap60,gz")
    ap.add_argument("--outputs", default="packed,xz")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    ref_fa, forms, n = write_inputs(a.dir, a.queries)
    cmds = {"parent": [os.path.join(a.parent_bin, "uvaialign")], "default": [os.path.join(ROOT, "bin", "uvaialign")],
            "device_parse": [os.path.join(ROOT, "bin", "uvaialign"), "--device-parse"]}
    result = {"queries": n, "rounds": a.rounds, "outputs": {}, "cold_cache": "not measured"}
    for output in a.outputs.split(","):
        result["outputs"][output] = {}
        for form in a.forms.split(","):
            path = forms[form]
            stem = {k: os.path.join(a.dir, "%s.%s.%s" % (output, form, k)) for k in cmds}
            out = {k: stem[k] + (".uvdb" if output == "packed" else ".aln.xz") for k in cmds}
            wall, dev = {k: [] for k in cmds}, []
            for rnd in range(a.rounds + 1):                 # round 0 warms the page cache and the GPU's clocks and is not counted
                for k, c in cmds.items():
                    w, d = run(c + ["-r", ref_fa, "-a", "1.0"] + (["--packed", out[k]] if output == "packed" else ["-o", stem[k]]) + [path])
                    sys.stderr.write("%s %s round %d %s: %.3f s\n" % (output, form, rnd, k, w))
                    sys.stderr.flush()
                    if rnd:
                        wall[k].append(w)
                        if d:
                            dev.append(d)
            one = {"bytes": os.path.getsize(path), "same_files": filecmp.cmp(out["parent"], out["default"], shallow=False) and filecmp.cmp(out["parent"], out["device_parse"], shallow=False),
                   "wall_s": {k: spread(v) for k, v in wall.items()}}
            p = one["wall_s"]["parent"]
            width = p["max"] - p["min"]
            one["default_not_slower_than_parent_beyond_its_spread"] = one["wall_s"]["default"]["median"] <= p["median"] + width
            one["device_parse_faster_than_default_beyond_parents_spread"] = one["wall_s"]["device_parse"]["median"] < one["wall_s"]["default"]["median"] - width
            if dev:
                one["device"] = {k: round(statistics.median(d[k] for d in dev), 3) for k in ("scan_ms", "count_ms", "sequences_ms", "align_ms")}
                one["device"]["text_bytes"] = dev[0]["bytes"]
            result["outputs"][output][form] = one
    print(json.dumps(result))


if __name__ == "__main__":
    main()
