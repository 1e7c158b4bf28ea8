#!/usr/bin/env python3
"""`uvaiapack --device-parse` against `uvaiapack` and against the parent commit's `uvaiapack` on the GPU box: the generator genomes of
tools/ingest_bench.py as plain FASTA with one line per sequence, plain FASTA wrapped at 60, .xz and .gz; one warming round, then counted
rounds that alternate the three commands on the same file.  Every pair of output files is compared.  Prints one JSON line.
profiles/device_parse.json is not such a line but holds two of them, of a run with --forms plain,wrap60 and one with --forms xz,gz, as
the entries of "runs" (each with the "forms_arg" it was started with), next to "tool", "parent", "where" and "note", which were written by hand.
Usage: python tools/device_parse_bench.py --parent-bin <parent checkout>/bin [--refs 100000] [--rounds 3] [--dir /tmp/device_parse]"""
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
from uvaia_amd import hostlib  # noqa: E402


def write_fasta(path, gen, refs, wrap):
    with open(path, "wb") as fh:
        for first in range(0, refs, 2048):
            rows, _ = gen.generate(first, min(2048, refs - first))
            n, nchar = rows.shape
            full = nchar // wrap if wrap else 0        # whole lines of `wrap` sites with their '\n', then the short last line
            body = np.concatenate([rows[:, :full * wrap].reshape(n, full, wrap), np.full((n, full, 1), 10, dtype=np.uint8)], axis=2).reshape(n, -1) if full else None
            for i in range(n):
                fh.write(b">ref_%d\n" % (first + i))
                if full:
                    fh.write(body[i].tobytes())
                if full * wrap < nchar:
                    fh.write(rows[i, full * wrap:].tobytes() + b"\n")


def cached_fraction(path):
    """the share of the file's pages in the page cache by fincore, None where the tool is missing"""
    try:
        out = subprocess.run(["fincore", "--bytes", "--noheadings", "--output", "RES,SIZE", path], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=60).stdout.split()
        return round(int(out[0]) / max(int(out[1]), 1), 3)
    except Exception:
        return None


def run(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    err = r.stderr.decode(errors="replace")
    if r.returncode:
        sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), err[-3000:]))
        sys.exit(1)
    read_s = sum(float(m) for m in re.findall(r"Finished reading file .* in ([0-9.]+) secs", err))
    dev = re.search(r"device parse: (\{.*\})", err)
    return wall, read_s, json.loads(dev.group(1)) if dev else None


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", required=True, help="bin/ of a built checkout of the parent commit")
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/device_parse")
    ap.add_argument("--forms", default="plain,wrap60,xz,gz")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    gen = hostlib.Synth()
    plain, wrap60 = os.path.join(a.dir, "refs.fa"), os.path.join(a.dir, "refs60.fa")
    write_fasta(plain, gen, a.refs, 0)
    forms = {"plain": plain}
    want = a.forms.split(",")
    if "wrap60" in want:
        write_fasta(wrap60, gen, a.refs, 60)
        forms["wrap60"] = wrap60
    if "xz" in want:
        subprocess.check_call("xz -T0 -1 -c %s > %s.xz" % (plain, plain), shell=True)
        forms["xz"] = plain + ".xz"
    if "gz" in want:
        subprocess.check_call("gzip -1 -c %s > %s.gz" % (plain, plain), shell=True)
        forms["gz"] = plain + ".gz"
    cmds = {"parent": [os.path.join(a.parent_bin, "uvaiapack")], "default": [os.path.join(ROOT, "bin", "uvaiapack")],
            "device_parse": [os.path.join(ROOT, "bin", "uvaiapack"), "--device-parse"]}
    result = {"refs": a.refs, "rounds": a.rounds, "forms": {}, "cold_cache": "not measured", "ten_million_genomes": "not measured"}
    for form in want:
        path = forms[form]
        out = {k: os.path.join(a.dir, "%s.%s.uvdb" % (form, k)) for k in cmds}
        wall, read, dev = {k: [] for k in cmds}, {k: [] for k in cmds}, []
        for rnd in range(a.rounds + 1):                 # round 0 warms the page cache and the GPU's clocks and is not counted
            for k, c in cmds.items():
                w, r, d = run(c + ["-o", out[k], path])
                sys.stderr.write("%s round %d %s: %.3f s\n" % (form, rnd, k, w))
                sys.stderr.flush()
                if rnd:
                    wall[k].append(w); read[k].append(r)
                    if d:
                        dev.append(d)
        one = {"bytes": os.path.getsize(path), "page_cache_fraction_after": cached_fraction(path),
               "same_files": filecmp.cmp(out["parent"], out["default"], shallow=False) and filecmp.cmp(out["parent"], out["device_parse"], shallow=False),
               "wall_s": {k: spread(v) for k, v in wall.items()}, "finished_reading_s": {k: spread(v) for k, v in read.items()}}
        p = one["wall_s"]["parent"]
        width = p["max"] - p["min"]
        one["default_not_slower_than_parent_beyond_its_spread"] = one["wall_s"]["default"]["median"] <= p["median"] + width
        one["device_parse_faster_than_parent_beyond_its_spread"] = one["wall_s"]["device_parse"]["median"] < p["median"] - width
        if dev:
            text = dev[0]["bytes"]
            scan, rows = statistics.median(d["scan_ms"] for d in dev), statistics.median(d["rows_ms"] for d in dev)
            one["device"] = {"text_bytes": text, "scan_ms": round(scan, 3), "rows_ms": round(rows, 3), "scan_gb_s": round(text / scan * 1e-6, 1), "rows_gb_s": round(text / rows * 1e-6, 1)}
        if form in ("xz", "gz"):
            tool = "xz" if form == "xz" else "gzip"
            ts = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                subprocess.check_call("%s -dc %s > /dev/null" % (tool, path), shell=True)
                ts.append(time.perf_counter() - t0)
            one["decompressor_alone_s"] = spread(ts)
        result["forms"][form] = one
    print(json.dumps(result))


if __name__ == "__main__":
    main()
