#!/usr/bin/env python3
"""`uvaia -r --device-parse` and `uvaiaclust --device-parse` against the same commands without the option and against the parent commit's
binaries on the GPU box, alternating in one session: one warming round, then counted rounds.  Every pair of output files is compared by
decompressed content.
  uvaia:      the generator genomes of tools/ingest_bench.py as plain FASTA with one line per sequence, wrapped at 60, and .gz; the first
              --queries of them as queries, -n 100 -p 65536.
  uvaiaclust: -d 3 -p 64 over synthetic families (tests/cluster_lib.py), with the peak resident host memory of each command (ru_maxrss).
Prints one JSON line; profiles/search_device_parse.json holds such lines as the entries of "runs", next to "tool", "parent", "where" and
"note", which were written by hand.
Usage: python tools/search_parse_bench.py --parent-bin <parent checkout>/bin [--refs 100000] [--queries 1000] [--rounds 3] [--dir /tmp/search_parse]
       [--forms plain,wrap60,gz] [--what uvaia,uvaiaclust]"""
import argparse
import json
import lzma
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from uvaia_amd import hostlib  # noqa: E402
from device_parse_bench import cached_fraction, spread, write_fasta  # noqa: E402


def run(cmd):
    """(wall seconds, peak resident host memory in KiB, stderr) of one command"""
    with tempfile.TemporaryFile() as err:
        t0 = time.perf_counter()
        p = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=err)
        _pid, status, usage = os.wait4(p.pid, 0)
        wall = time.perf_counter() - t0
        p.returncode = os.waitstatus_to_exitcode(status)
        err.seek(0)
        text = err.read().decode(errors="replace")
    if p.returncode:
        sys.stderr.write("FAILED (%d): %s\n%s\n" % (p.returncode, " ".join(cmd), text[-3000:]))
        sys.exit(1)
    return wall, usage.ru_maxrss, text


def same_outputs(prefixes, suffixes=(".csv.xz", ".aln.xz")):
    first = [lzma.open(prefixes[0] + s).read() for s in suffixes]
    return all([lzma.open(p + s).read() for s in suffixes] == first for p in prefixes[1:])


def measure(cmds, rounds, label, outputs):
    """cmds: {name: argv without -o}; alternates them for rounds + 1 rounds (round 0 warms the page cache and the GPU's clocks and is not counted)"""
    wall, rss, dev, read = {k: [] for k in cmds}, {k: [] for k in cmds}, [], {k: [] for k in cmds}
    for rnd in range(rounds + 1):
        for k, c in cmds.items():
            w, m, err = run(c + ["-o", outputs[k]])
            sys.stderr.write("%s round %d %s: %.3f s, %d KiB\n" % (label, rnd, k, w, m))
            sys.stderr.flush()
            if rnd:
                wall[k].append(w); rss[k].append(m)
                read[k].append(sum(float(x) for x in re.findall(r"Finished reading file .* in ([0-9.]+) secs", err)))
                d = re.search(r"device parse: (\{.*\})", err)
                if d:
                    dev.append(json.loads(d.group(1)))
    one = {"same_outputs": same_outputs([outputs[k] for k in cmds]), "wall_s": {k: spread(v) for k, v in wall.items()},
           "finished_reading_s": {k: spread(v) for k, v in read.items()}, "peak_host_rss_kib": {k: spread(v) for k, v in rss.items()}}
    p = one["wall_s"]["parent"]
    width = p["max"] - p["min"]
    one["default_not_slower_than_parent_beyond_its_spread"] = one["wall_s"]["default"]["median"] <= p["median"] + width
    one["device_parse_faster_than_parent_beyond_its_spread"] = one["wall_s"]["device_parse"]["median"] < p["median"] - width
    if dev:
        one["device"] = {k: round(statistics.median(d[k] for d in dev), 3) for k in dev[0] if k.endswith("_ms")}
        one["device"].update({k: dev[0][k] for k in ("bytes", "block_bytes", "window") if k in dev[0]})
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", required=True, help="bin/ of a built checkout of the parent commit")
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/search_parse")
    ap.add_argument("--forms", default="plain,wrap60,gz")
    ap.add_argument("--what", default="uvaia,uvaiaclust")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    what = a.what.split(",")
    result = {"refs": a.refs, "queries": a.queries, "rounds": a.rounds, "cold_cache": "not measured", "ten_million_genomes": "not measured"}
    names = ("parent", "default", "device_parse")
    if "uvaia" in what:
        gen = hostlib.Synth()
        plain, wrap60, query = os.path.join(a.dir, "refs.fa"), os.path.join(a.dir, "refs60.fa"), os.path.join(a.dir, "queries.fa")
        write_fasta(plain, gen, a.refs, 0)
        write_fasta(query, gen, a.queries, 0)
        forms, want = {"plain": plain}, a.forms.split(",")
        if "wrap60" in want:
            write_fasta(wrap60, gen, a.refs, 60)
            forms["wrap60"] = wrap60
        if "gz" in want:
            subprocess.check_call("gzip -1 -c %s > %s.gz" % (plain, plain), shell=True)
            forms["gz"] = plain + ".gz"
        result["uvaia"] = {"options": "-n 100 -p 65536", "forms": {}}
        for form in want:
            path = forms[form]
            tail = ["-n", "100", "-p", "65536", "-r", path, query]
            cmds = {"parent": [os.path.join(a.parent_bin, "uvaia")] + tail, "default": [os.path.join(ROOT, "bin", "uvaia")] + tail,
                    "device_parse": [os.path.join(ROOT, "bin", "uvaia"), "--device-parse"] + tail}
            one = measure(cmds, a.rounds, "uvaia " + form, {k: os.path.join(a.dir, "uvaia_%s_%s" % (form, k)) for k in names})
            one["bytes"], one["page_cache_fraction_after"] = os.path.getsize(path), cached_fraction(path)
            if form == "gz":
                ts = []
                for _ in range(a.rounds):
                    t0 = time.perf_counter()
                    subprocess.check_call("gzip -dc %s > /dev/null" % path, shell=True)
                    ts.append(time.perf_counter() - t0)
                one["decompressor_alone_s"] = spread(ts)
            result["uvaia"]["forms"][form] = one
    if "uvaiaclust" in what:
        import cluster_lib as CL
        fam = CL.families(a.refs, a.refs // 13, 20261017)
        path = os.path.join(a.dir, "families.fa")
        with open(path, "wb") as fh:
            for i, s in enumerate(fam):
                fh.write(b">fam_%d\n" % i + s + b"\n")
        del fam
        tail = ["-d", "3", "-p", "64", path]
        cmds = {"parent": [os.path.join(a.parent_bin, "uvaiaclust")] + tail, "default": [os.path.join(ROOT, "bin", "uvaiaclust")] + tail,
                "device_parse": [os.path.join(ROOT, "bin", "uvaiaclust"), "--device-parse"] + tail}
        one = measure(cmds, a.rounds, "uvaiaclust", {k: os.path.join(a.dir, "clust_%s" % k) for k in names})
        one["bytes"], one["options"], one["page_cache_fraction_after"] = os.path.getsize(path), "-d 3 -p 64", cached_fraction(path)
        result["uvaiaclust"] = one
    print(json.dumps(result))


if __name__ == "__main__":
    main()
