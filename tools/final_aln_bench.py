#!/usr/bin/env python3
"""Rows out of a packed database on the GPU box: `uvaia --packed --final-aln [--final-only]` next to the plain command and to the parent
commit's, and `uvaiapack --unpack` of a dense and of a compact file.  The workload is tools/compact_bench.py's: generator genomes
(SARS-CoV-2 length), 1 000 queries, pool 8 192, -n 100, on the dense file.  One warming round (it reads the files into the page cache and
is not counted), then `--repeats` counted rounds in which the commands alternate, every round starting one command further on (so that no
command always follows the same neighbour):
  a  the parent commit's `uvaia --packed`                 (--parent-bin; the yardstick)
  b  this tree's, same arguments                          outputs compared with a's, decompressed
  c  this tree's with --final-aln                         regular outputs compared with a's; the final file with the filter of a's outputs
  d  this tree's with --final-aln --final-only            table compared with a's; the final file as for c; no <prefix>.aln.xz
each resident and with --window 25000, and `uvaiapack --unpack --stdout > /dev/null` of both files.
Reported as measured: wall times (median, min, max), references dumped against final members, the parts of an extraction (staging calls,
decode kernel, copy back, exception runs, write), and whether b's median is within a's own min-max spread of a's median (the bar for a
pull request that moves code in that path).  The bar is reported, not asserted; unequal outputs (or a <prefix>.aln.xz that --final-only
left) are: the tool then writes the profile to <out>.rejected and exits with status 1, so that such a profile cannot be kept unnoticed.
Writes profiles/final_aln.json and prints it.
Usage: python tools/final_aln_bench.py --parent-bin <parent checkout>/bin [--refs 100000] [--queries 1000] [--dir /tmp/final_aln_bench]"""
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


def spread(xs):
    return {"median_s": round(statistics.median(xs), 3), "min_s": round(min(xs), 3), "max_s": round(max(xs), 3), "all_s": [round(x, 3) for x in xs]}


STAGES = (("read_queries_s", r"Finished reading \d+ query references in ([0-9.]+) secs"), ("load_s", r"Loaded \d+ packed sequences from .* in ([0-9.]+) secs"),
          ("search_and_dump_s", r"Saved \d+ sequences to file \S+ , ([0-9.]+) secs elapsed"), ("table_s", r"Saved distance table to file \S+ , ([0-9.]+) secs elapsed"),
          ("final_s", r"Saved \d+ sequences of the final neighbour lists to file \S+ , ([0-9.]+) secs elapsed"))


def stages(err):
    """the command's own figures: each is the time since the figure before it (query preparation and engine start-up fall to load_s' predecessor
    and to search_and_dump_s, which also waits for xz to finish the dump)"""
    out = {}
    for key, pat in STAGES:
        m = re.search(pat, err)
        if m:
            out[key] = float(m.group(1))
    return out


def expected_final(prefix, rank):
    """the test's filter: the records of <prefix>.aln.xz whose name is in column 2 of <prefix>.csv.xz with rank <= rank, in file order"""
    names = set()
    for line in lzma.open(prefix + ".csv.xz", "rb").read().split(b"\n")[1:]:
        if line:
            cols = line.split(b",")
            if int(cols[2]) <= rank:
                names.add(cols[1])
    lines = lzma.open(prefix + ".aln.xz", "rb").read().split(b"\n")
    out = [h + b"\n" + s + b"\n" for h, s in zip(lines[0:-1:2], lines[1:-1:2]) if h[1:] in names]
    return b"".join(out), len(out), (len(lines) - 1) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dir", default="/tmp/final_aln_bench")
    ap.add_argument("--pool", type=int, default=8192)
    ap.add_argument("--nbest", type=int, default=100)
    ap.add_argument("--window", type=int, default=25000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-bin", default=None, help="directory with the parent commit's uvaia (command a); without it b is its own yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "final_aln.json"))
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    gen = hostlib.Synth()
    uv, pk = os.path.join(ROOT, "bin", "uvaia"), os.path.join(ROOT, "bin", "uvaiapack")

    def run(cmd, stdout=subprocess.DEVNULL):
        sys.stderr.write("running %s\n" % " ".join(cmd[:1] + cmd[-4:])); sys.stderr.flush()
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=stdout, stderr=subprocess.PIPE)
        wall = time.perf_counter() - t0
        err = r.stderr.decode(errors="replace")
        if r.returncode:
            sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), err[-3000:]))
            sys.exit(1)
        return wall, err

    fa, dense, compact, q_fa = (os.path.join(a.dir, x) for x in ("refs.fa", "dense.uvdb", "compact.uvdb", "query.fa"))
    with open(fa, "wb") as fh:
        for first in range(0, a.refs, 2048):
            rows, _ = gen.generate(first, min(2048, a.refs - first))
            for i in range(rows.shape[0]):
                fh.write(b">ref_%d\n" % (first + i) + rows[i].tobytes() + b"\n")
    run([pk, "-o", dense, fa])
    run([pk, "--compact", "-o", compact, fa])
    os.remove(fa)
    with open(q_fa, "wb") as fh:
        rows, _ = gen.generate(10_000_000, a.queries)
        for i in range(rows.shape[0]):
            fh.write(b">q_%d\n" % i + rows[i].tobytes() + b"\n")

    kinds = [("b_plain", uv, []), ("c_final", uv, ["--final-aln"]), ("d_final_only", uv, ["--final-aln", "--final-only"])]
    if a.parent_bin:
        kinds.insert(0, ("a_parent", os.path.join(a.parent_bin, "uvaia"), []))
    yard = kinds[0][0]
    modes = {"resident": [], "window": ["--window", str(a.window)]}
    prefix = lambda mode, kind: os.path.join(a.dir, "out_%s_%s" % (mode, kind))
    walls = {m: {k: [] for k, _, _ in kinds} for m in modes}
    reports = {m: {k: [] for k, _, _ in kinds} for m in modes}
    staged = {m: {k: [] for k, _, _ in kinds} for m in modes}
    unpack = {"dense": {"wall": [], "report": []}, "compact": {"wall": [], "report": []}}
    devnull = open(os.devnull, "wb")
    for rep in range(a.repeats + 1):
        for mode, extra in modes.items():
            for kind, exe, opts in kinds[rep % len(kinds):] + kinds[:rep % len(kinds)]:
                wall, err = run([exe, q_fa, "-p", str(a.pool), "-n", str(a.nbest), "-o", prefix(mode, kind), "--window-report"] + extra + opts + ["--packed", dense])
                if rep:
                    walls[mode][kind].append(wall)
                    staged[mode][kind].append(stages(err))
                    m = re.search(r"final report: (\{.*\})", err)
                    reports[mode][kind].append(json.loads(m.group(1)) if m else None)
        for kind, db in (("dense", dense), ("compact", compact)):
            wall, err = run([pk, "--unpack", "--stdout", db], stdout=devnull)
            if rep:
                unpack[kind]["wall"].append(wall)
                unpack[kind]["report"].append(json.loads(re.search(r"unpack report: (\{.*\})", err).group(1)))

    result = {"refs": a.refs, "queries": a.queries, "pool": a.pool, "nbest": a.nbest, "window": a.window, "repeats": a.repeats, "file": "dense", "commands": {}}
    xz = lambda p, s: lzma.open(p + s, "rb").read()
    for mode in modes:
        want_csv, want_aln = xz(prefix(mode, yard), ".csv.xz"), xz(prefix(mode, yard), ".aln.xz")
        want_final, n_final, n_dumped = expected_final(prefix(mode, yard), a.nbest)
        res = {"references_dumped": n_dumped, "final_members": n_final}
        for kind, _, opts in kinds:
            e = dict(spread(walls[mode][kind]))
            e["stages_median_s"] = {k: round(statistics.median(r[k] for r in staged[mode][kind] if k in r), 3) for k, _ in STAGES if any(k in r for r in staged[mode][kind])}
            e["table_equal_%s" % yard] = xz(prefix(mode, kind), ".csv.xz") == want_csv
            if "--final-only" in opts:
                e["regular_alignment_written"] = os.path.exists(prefix(mode, kind) + ".aln.xz")
            else:
                e["alignment_equal_%s" % yard] = xz(prefix(mode, kind), ".aln.xz") == want_aln
            if opts:
                e["final_equal_filter_of_%s" % yard] = xz(prefix(mode, kind), ".final.aln.xz") == want_final
                rp = [r for r in reports[mode][kind] if r]
                e["extraction"] = {k: round(statistics.median(r[k] for r in rp), 3) for k in rp[0]} if rp else None
            res[kind] = e
        ya, b = res[yard], res["b_plain"]
        res["bar"] = {"yardstick": yard, "yardstick_spread_s": round(ya["max_s"] - ya["min_s"], 3), "b_median_minus_yardstick_median_s": round(b["median_s"] - ya["median_s"], 3),
                      "met": b["median_s"] - ya["median_s"] <= ya["max_s"] - ya["min_s"]}
        res["d_over_yardstick_median"] = round(res["d_final_only"]["median_s"] / ya["median_s"], 3)
        result["commands"][mode] = res
    result["unpack"] = {}
    for kind, u in unpack.items():
        med = {k: statistics.median(r[k] for r in u["report"]) for k in u["report"][0]}
        per_m = 1e6 / max(med["rows"], 1)
        result["unpack"][kind] = dict(spread(u["wall"]), report_median={k: round(v, 3) for k, v in med.items()},
                                      decode_kernel_ms_per_million_refs=round(med["decode_kernel_ms"] * per_m, 1),
                                      copy_back_ms_per_million_refs=round((med["decode_ms"] - med["decode_kernel_ms"]) * per_m, 1))
    result["note"] = ("wall clock of the whole commands (query preparation, engine start-up, xz output included); page cache WARM for both files (round 0 of the "
                      "alternation reads them and is not counted); extraction: medians of the commands' own 'final report' / 'unpack report' lines -- stage_ms, "
                      "decode_ms, exceptions_ms and write_ms are host wall time of the staging calls, of the decode calls (kernel, copy back to the host and the wait "
                      "for both), of the exception runs and of the receiver (FASTA formatting, xz or the write to /dev/null); decode_kernel_ms is device time "
                      "(HIP events around unpack_rows_kernel); copy back = decode_ms - decode_kernel_ms")
    wrong = ["%s %s %s" % (mode, kind, k) for mode, res in result["commands"].items() for kind, e in res.items() if isinstance(e, dict)
             for k, v in e.items() if (("_equal_" in k and v is not True) or (k == "regular_alignment_written" and v))]
    if wrong:
        a.out += ".rejected"
        sys.stderr.write("OUTPUTS DIFFER: %s\n" % "; ".join(wrong))
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))
    if wrong:
        sys.exit(1)


if __name__ == "__main__":
    main()
