#!/usr/bin/env python3
"""`uvaia --packed` resident against `uvaia --packed --window` on the GPU box: the whole command over the synthetic database of
tools/ingest_bench.py (100 000 references, 1 000 queries), resident and with windows of 16 384 and 32 768 references, alternating, three
repeats, medians.  Records whether the output files are identical, the device time of the three window steps (uvaia_gpu_window_ms), the
share of the upload that ran next to a search, and the free device memory before the database and after the search for every command.
Writes profiles/nearest_window.json and prints it.
Usage: python tools/window_bench.py [--refs 100000] [--queries 1000] [--dir /tmp/window_bench] [--out profiles/nearest_window.json]"""
import argparse
import json
import lzma
import os
import re
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
    ap.add_argument("--dir", default="/tmp/window_bench")
    ap.add_argument("--pool", type=int, default=8192)
    ap.add_argument("--windows", default="16384,32768")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_window.json"))
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    gen = hostlib.Synth()
    ref_fa, q_fa, db = (os.path.join(a.dir, x) for x in ("refs.fa", "query.fa", "refs.uvdb"))
    with open(ref_fa, "wb") as fh:
        for first in range(0, a.refs, 2048):
            rows, _ = gen.generate(first, min(2048, a.refs - first))
            for i in range(rows.shape[0]):
                fh.write(b">ref_%d\n" % (first + i) + rows[i].tobytes() + b"\n")
    with open(q_fa, "wb") as fh:
        rows, _ = gen.generate(10_000_000, a.queries)
        for i in range(rows.shape[0]):
            fh.write(b">q_%d\n" % i + rows[i].tobytes() + b"\n")
    uv, pk = os.path.join(ROOT, "bin", "uvaia"), os.path.join(ROOT, "bin", "uvaiapack")

    def run(cmd):
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if r.returncode:
            sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), r.stderr.decode(errors="replace")[-3000:]))
            sys.exit(1)
        return time.perf_counter() - t0, r.stderr.decode(errors="replace")

    run([pk, "-o", db, ref_fa])
    os.remove(ref_fa)
    configs = [0] + [int(w) for w in a.windows.split(",")]
    secs, reports = {w: [] for w in configs}, {}
    for rep in range(a.repeats + 1):                        # the first round warms the page cache and is not counted
        for w in configs:
            out = os.path.join(a.dir, "out_%d" % w)
            cmd = [uv, "--packed", db, q_fa, "-p", str(a.pool), "-n", "100", "-o", out, "--window-report"] + (["--window", str(w)] if w else [])
            t, log = run(cmd)
            if rep:
                secs[w].append(t)
            reports[w] = json.loads(re.search(r"window report: (\{.*\})", log).group(1))
    content = {w: [lzma.open(os.path.join(a.dir, "out_%d%s" % (w, s)), "rb").read() for s in (".csv.xz", ".aln.xz")] for w in configs}
    med = {w: statistics.median(secs[w]) for w in configs}
    result = {"refs": a.refs, "queries": a.queries, "pool": a.pool, "repeats": a.repeats, "uvdb_bytes": os.path.getsize(db),
              "resident": {"median_s": round(med[0], 3), "all_s": [round(x, 3) for x in secs[0]], "report": reports[0]},
              "windowed": {str(w): {"median_s": round(med[w], 3), "all_s": [round(x, 3) for x in secs[w]], "ratio_to_resident": round(med[w] / med[0], 3),
                                    "files_identical": content[w] == content[0], "report": reports[w],
                                    "device_bytes_taken": reports[w]["free_before"] - reports[w]["free_after"]} for w in configs[1:]},
              "resident_device_bytes_taken": reports[0]["free_before"] - reports[0]["free_after"],
              "note": "wall clock of the whole command (query preparation, engine start-up, xz output included), page cache warm; free_before / free_after: "
                      "hipMemGetInfo before the database is reserved and after the search; report times in ms, device time of the window steps"}
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
