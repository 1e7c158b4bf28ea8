#!/usr/bin/env python3
"""Several packed databases as one on the GPU box: one synthetic database (tools/ingest_bench.py's generator) packed as 1, 4 and 16 files of
equal share, then for every cut the whole command `uvaia --packed f0 --packed f1 ...` (resident load of all files, search, output) and
`uvaiapack --merge` of the files (references per second), alternating, medians over the repeats.  The cut into one file is the single-file
command: the same code as the other cuts, a set of one file, whose chunks go to the engine straight from the mapping.  It is the figure to
hold the others against, and the one to hold against the parent commit's (its --single-only run on the same box).  With --same-names K,
K queries are named like references spread over the database and every command gets -x: the kept stream has holes, so one file too is
staged and selected on the device.  Records whether every cut gives the single file's outputs and whether every merge gives its bytes.
Writes profiles/packed_set.json and prints it.
Usage: python tools/packed_set_bench.py [--refs 100000] [--queries 1000] [--dir /tmp/packed_set_bench] [--out profiles/packed_set.json] [--single-only]
       [--same-names K] [--parent-single-file-s <seconds>]   (the search_median_s a --single-only run on the parent commit printed)"""
import argparse
import json
import lzma
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uvaia_amd import hostlib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dir", default="/tmp/packed_set_bench")
    ap.add_argument("--pool", type=int, default=8192)
    ap.add_argument("--cuts", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--single-only", action="store_true", help="only the single-file command (what a commit without the set code can run)")
    ap.add_argument("--same-names", type=int, default=0, help="name this many queries like references spread over the database and pass -x")
    ap.add_argument("--parent-single-file-s", type=float, default=None, help="median of the single-file command on the parent commit (its --single-only run on the same box): recorded next to the cuts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_set.json"))
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    gen = hostlib.Synth()
    uv, pk = os.path.join(ROOT, "bin", "uvaia"), os.path.join(ROOT, "bin", "uvaiapack")
    cuts = [1] if a.single_only else [int(c) for c in a.cuts.split(",")]

    def run(cmd):
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if r.returncode:
            sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), r.stderr.decode(errors="replace")[-3000:]))
            sys.exit(1)
        return time.perf_counter() - t0

    q_fa = os.path.join(a.dir, "query.fa")
    with open(q_fa, "wb") as fh:
        rows, _ = gen.generate(10_000_000, a.queries)
        for i in range(rows.shape[0]):
            name = b"ref_%d" % (i * a.refs // a.same_names) if i < a.same_names else b"q_%d" % i
            fh.write(b">" + name + b"\n" + rows[i].tobytes() + b"\n")
    exclude = ["-x"] if a.same_names else []
    files = {}
    for c in cuts:                                          # file k of a cut into c holds references [k * share, (k + 1) * share): no multiple of 64 unless the share is
        share, files[c] = -(-a.refs // c), []
        for k in range(c):
            fa, db = os.path.join(a.dir, "cut%d_%d.fa" % (c, k)), os.path.join(a.dir, "cut%d_%d.uvdb" % (c, k))
            with open(fa, "wb") as fh:
                for first in range(k * share, min(a.refs, (k + 1) * share), 2048):
                    rows, _ = gen.generate(first, min(2048, min(a.refs, (k + 1) * share) - first))
                    for i in range(rows.shape[0]):
                        fh.write(b">ref_%d\n" % (first + i) + rows[i].tobytes() + b"\n")
            run([pk, "-o", db, fa])
            os.remove(fa)
            files[c].append(db)
    search, merge = {c: [] for c in cuts}, {c: [] for c in cuts}
    for rep in range(a.repeats + 1):                        # the first round warms the page cache and is not counted
        for c in cuts:
            t = run([uv, q_fa, "-p", str(a.pool), "-n", "100", "-o", os.path.join(a.dir, "out_%d" % c)] + exclude + [x for f in files[c] for x in ("--packed", f)])
            if rep:
                search[c].append(t)
            if not a.single_only:
                t = run([pk, "--merge", "-o", os.path.join(a.dir, "merged_%d.uvdb" % c)] + files[c])
                if rep:
                    merge[c].append(t)
    content = {c: [lzma.open(os.path.join(a.dir, "out_%d%s" % (c, s)), "rb").read() for s in (".csv.xz", ".aln.xz")] for c in cuts}
    single = open(files[1][0], "rb").read() if 1 in cuts and not a.single_only else None
    result = {"refs": a.refs, "queries": a.queries, "pool": a.pool, "repeats": a.repeats, "same_names": a.same_names, "cuts": {}}
    for c in cuts:
        e = {"files": c, "search_median_s": round(statistics.median(search[c]), 3), "search_all_s": [round(x, 3) for x in search[c]],
             "outputs_equal_single_file": content[c] == content[cuts[0]]}
        if merge[c]:
            m = statistics.median(merge[c])
            e.update({"merge_median_s": round(m, 3), "merge_all_s": [round(x, 3) for x in merge[c]], "merge_refs_per_s": round(a.refs / m),
                      "merge_equals_single_file": (open(os.path.join(a.dir, "merged_%d.uvdb" % c), "rb").read() == single) if single is not None else None})
        result["cuts"][str(c)] = e
    result["note"] = ("wall clock of the whole commands (query preparation, engine start-up, xz output included), page cache warm; the cut into 1 file runs "
                      "the same code as a set of one file (without -x its chunks go straight from the mapping, as on the parent); same_names > 0: "
                      "that many queries named like references and -x; parent_single_file_s: the same command on the parent commit, where it was run")
    result["parent_single_file_s"] = a.parent_single_file_s
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
