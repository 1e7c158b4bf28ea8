#!/usr/bin/env python3
"""Single-linkage clusters on the device (uvaia_gpu_db_link_*, kernels_pairs.inc) on the GPU box.  The numbers are recorded; what is checked
is only that the link forms agree with each other (links == the threshold form's count, the dense case is one cluster).
  (a) link kernels   generator genomes (host/synth.c, SARS-CoV-2 length) resident in one engine; device time (uvaia_gpu_link_ms) of the snp link
                     kernel with the floor off and on over rows [0, --rows) x columns [0, --refs), next to pairs_snp_kernel<32> over the same
                     rectangle (uvaia_gpu_pairs_ms); D = 2 over rows [0, --within-rows) x columns [0, --within-refs) next to the threshold
                     form (uvaia_gpu_db_pairs_within); one warming round, --rounds counted ones, median and min-max
  (b) the parent     with --parent-lib <libuvaia_gpu.so of the parent commit>: the dense snp kernel and the threshold form from that library,
                     in processes of their own that alternate with this tree's
  (c) dense case     --rows identical rows at D = 0 (every lane hits every row: the union's worst case) against the same kernel on the
                     generator's rows at D = 0
  (d) whole command  `uvaiadist --packed -d 2 --clusters` against `uvaiadist --packed -d 2` of the --refs rows, to /dev/null
Writes profiles/pair_link.json and prints it.
Usage: python tools/pair_link_bench.py [--parent-lib PATH] [--refs 20000] [--rows 4096] [--within-refs 100000] [--within-rows 8192] [--dir /tmp/pair_link]"""
import argparse
import ctypes as C
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


def spread(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "all_ms": [round(x, 3) for x in v]}


class _Absent:
    """stands in for an entry a library of the parent commit does not have (its signature is set and never called)"""
    restype = argtypes = None


class _Lenient:
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        try:
            return getattr(self._lib, name)
        except AttributeError:
            return _Absent()


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


def timed(rounds, reset, run, read):
    ms, last = [], None
    for r in range(rounds + 1):
        reset()
        last = run()
        if r:
            ms.append(read())
    return ms, last


def worker(a):
    """one process, one library: the measurements that library can make, as one JSON line"""
    parent = bool(a.lib)
    if parent:
        capi._LIB = a.lib
        cdll = C.CDLL
        C.CDLL = lambda path, *k, **kw: _Lenient(cdll(path, *k, **kw))
    res = {}
    n = max(a.refs, a.within_refs)
    with open_engine(a, n) as eng:
        out = np.zeros((a.rows, a.refs), dtype=np.int32)
        ms, _ = timed(a.rounds, lambda: eng.pairs_ms(reset=True), lambda: eng.db_pairs(rows=(0, a.rows), cols=(0, a.refs), out=out), lambda: eng.pairs_ms()["dense"])
        res["pairs_snp_kernel_32"] = dict(spread(ms), rows=a.rows, cols=a.refs)
        ms, last = timed(a.rounds, lambda: eng.pairs_ms(reset=True),
                         lambda: eng.db_pairs_within(2, rows=(0, a.within_rows), cols=(0, a.within_refs), metric=capi.DIST_SNP, upper=True, cap=1 << 22), lambda: eng.pairs_ms()["within"])
        res["within_d2_upper"] = dict(spread(ms), rows=a.within_rows, cols=a.within_refs, found=int(last[1]))
        if not parent:
            for key, floor in (("link_snp_floor_off", 0), ("link_snp_floor_on", 1)):
                def run(floor=floor):
                    eng.db_link_begin(2, min_compared=floor)
                    return eng.db_link(rows=(0, a.rows), cols=(0, a.refs))
                ms, links = timed(a.rounds, lambda: eng.link_ms(reset=True), run, eng.link_ms)
                res[key] = dict(spread(ms), rows=a.rows, cols=a.refs, max_dist=2, min_compared=floor, links=links)

            def run_within():
                eng.db_link_begin(2)
                return eng.db_link(rows=(0, a.within_rows), cols=(0, a.within_refs))
            ms, links = timed(a.rounds, lambda: eng.link_ms(reset=True), run_within, eng.link_ms)
            labels = eng.db_link_labels()
            res["link_d2"] = dict(spread(ms), rows=a.within_rows, cols=a.within_refs, links=links, clusters=int(len(np.unique(labels))),
                                  links_equal_the_threshold_forms_count=bool(links == res["within_d2_upper"]["found"]))

            def run_sparse():
                eng.db_link_begin(0)
                return eng.db_link(rows=(0, a.rows), cols=(0, a.rows))
            ms, links = timed(a.rounds, lambda: eng.link_ms(reset=True), run_sparse, eng.link_ms)
            res["generator_rows_d0"] = dict(spread(ms), rows=a.rows, cols=a.rows, links=links)
    if not parent:
        import oracle_lib as O
        gen = hostlib.Synth()
        rows, non_n = gen.generate(0, 1)
        root = bytes(b"ACGT"[s & 3] for s in range(NCHAR))
        with capi.Engine.from_query(O.Query([root], ["q"]), nbest=1, max_pool=64, device=a.device) as eng:
            eng.db_reserve(a.rows)
            block, nn = np.repeat(rows, 4096, axis=0), np.repeat(non_n, 4096)
            for first in range(0, a.rows, 4096):
                m = min(4096, a.rows - first)
                eng.db_append_block(np.ascontiguousarray(block[:m]), np.ascontiguousarray(nn[:m]))

            def run_dense():
                eng.db_link_begin(0)
                return eng.db_link()
            ms, links = timed(a.rounds, lambda: eng.link_ms(reset=True), run_dense, eng.link_ms)
            labels = eng.db_link_labels()
            res["identical_rows_d0"] = dict(spread(ms), rows=a.rows, cols=a.rows, links=links, every_pair_linked=bool(links == a.rows * (a.rows - 1) // 2),
                                            one_cluster=bool(not labels.any()))
    print("RESULT " + json.dumps(res))


def run_worker(a, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--refs", a.refs, "--rows", a.rows, "--within-refs", a.within_refs, "--within-rows", a.within_rows,
           "--rounds", a.rounds, "--device", a.device] + (["--lib", lib] if lib else [])
    r = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode:
        raise RuntimeError("worker (%s) ended with %d: %s" % (lib or "this tree", r.returncode, r.stderr.decode()[-400:]))
    return json.loads(re.search(r"^RESULT (.*)$", r.stdout.decode(), re.M).group(1))


def kernels(a, doc):
    runs = {"parent": [], "this_tree": []}
    for _ in range(a.alternations):
        if a.parent_lib:
            runs["parent"].append(run_worker(a, os.path.abspath(a.parent_lib)))
        runs["this_tree"].append(run_worker(a, None))
    doc["alternating_runs"] = runs

    def med(side, key):
        return round(statistics.median(r[key]["median_ms"] for r in runs[side]), 3)

    def span(side, key):
        v = [x for r in runs[side] for x in r[key]["all_ms"]]
        return [min(v), max(v)]
    s = {}
    for key in ("link_snp_floor_off", "link_snp_floor_on", "link_d2", "generator_rows_d0", "identical_rows_d0", "pairs_snp_kernel_32", "within_d2_upper"):
        s[key] = {"median_ms": med("this_tree", key), "min_max_ms": span("this_tree", key)}
    for key in ("pairs_snp_kernel_32", "within_d2_upper"):
        if runs["parent"]:
            s["parent_" + key] = {"median_ms": med("parent", key), "min_max_ms": span("parent", key)}
    base = s.get("parent_pairs_snp_kernel_32", s["pairs_snp_kernel_32"])["median_ms"]
    s["floor_off_over_pairs_snp_kernel_32"] = round(s["link_snp_floor_off"]["median_ms"] / base, 3)
    s["floor_on_over_pairs_snp_kernel_32"] = round(s["link_snp_floor_on"]["median_ms"] / base, 3)
    s["link_d2_over_the_threshold_form"] = round(s["link_d2"]["median_ms"] / s.get("parent_within_d2_upper", s["within_d2_upper"])["median_ms"], 3)
    s["identical_over_generator_rows"] = round(s["identical_rows_d0"]["median_ms"] / s["generator_rows_d0"]["median_ms"], 3)
    doc["summary"] = s


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
    res = {"clusters": [], "pairs": []}
    for _ in range(a.command_rounds):
        for key, form in (("pairs", []), ("clusters", ["--clusters"])):
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(ROOT, "bin", "uvaiadist"), "-o", "/dev/null", "-d", "2"] + form + ["--packed", db], stderr=subprocess.PIPE, check=True)
            rep = json.loads(re.search(rb"dist report: (\{.*\})", r.stderr).group(1))
            rep["wall_s"] = round(time.perf_counter() - t0, 2)
            res[key].append(rep)
    doc["whole_command_d2_to_dev_null"] = res
    os.remove(db)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--within-refs", type=int, default=100000)
    ap.add_argument("--within-rows", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--command-rounds", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--dir", default="/tmp/pair_link")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_link.json"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    doc = {"nchar": NCHAR, "refs": a.refs, "rounds": a.rounds, "alternations": a.alternations, "parent_library": bool(a.parent_lib),
           "instructions_per_pair_word": {"pairs_snp_kernel_32": 4, "link_snp_floor_off": 4, "link_snp_floor_on": 6, "pairs_counts_kernel": 17}, "not_measured": []}
    for name, f in (("kernels", kernels), ("whole_command", whole_command)):
        try:
            f(a, doc)
            failed = None
        except Exception as e:       # what could not be run is named and nothing more is started; what was measured is still written
            failed = "%s and what follows it: %s" % (name, e)
            doc["not_measured"].append(failed)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        if failed:
            break
    print(json.dumps(doc))
    if doc["not_measured"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
