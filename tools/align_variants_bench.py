#!/usr/bin/env python3
"""What deriving substitutions, deletions and per-row counts costs on the GPU box: the workload of `bench.py --align-only` (BASELINE
config[4]: 10 000 unaligned generator genomes against one reference of 29 903 sites) through uvaia_align_run with uvaia_align_set_variants off
and on, alternating in one process on one resident pool -- and, with --parent-lib, the library of the parent commit in the same rounds on
a pool of its own --, and the whole command `uvaialign --packed` with and without `--variants --qc`, alternating, with a warm page cache.
The time of the passes (uvaia_align_variants_ms) is set against two reads of the pool's rows at the box's measured read-only rate
(profiles/r01_hbm_read_ceiling.txt) and against the aligner's own kernel time.  Rows, scores and cells with the option off and on are
compared, the records with the numpy restatement of tests/align_variants.py on a sample of rows, and the command's QC table with the
library's counts.  Prints one JSON line; profiles/align_variants.json holds such a line as "run", next to "tool", "where", "note" and
"device_code", which were written by hand.
Usage: python tools/align_variants_bench.py [--queries 10000] [--rounds 5] [--cli-rounds 3] [--parent-lib libuvaia_gpu.so] [--dir /tmp/align_variants]"""
import argparse
import ctypes as C
import filecmp
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import align_variants as AV  # noqa: E402
from align_insertions_bench import NCHAR, spread, workload  # noqa: E402
from uvaia_amd import align  # noqa: E402


def read_ceiling():
    """GB/s of the best streaming read on the box, as profiles/r01_hbm_read_ceiling.txt has it"""
    text = open(os.path.join(ROOT, "profiles", "r01_hbm_read_ceiling.txt")).read()
    return float(re.search(r"best ([0-9.]+) GB/s", text).group(1))


class ParentAligner:
    """load_block / run / stats of another build of the library (the parent's has no variant entries), on a pool of its own"""

    def __init__(self, path, ref, seqs):
        vp, pi = C.c_void_p, C.POINTER(C.c_int)
        self.L = L = C.CDLL(path)
        L.uvaia_align_open.argtypes = [C.POINTER(vp), C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        L.uvaia_align_close.argtypes = [vp]
        L.uvaia_align_close.restype = None
        L.uvaia_align_last_error.argtypes = [vp]
        L.uvaia_align_last_error.restype = C.c_char_p
        L.uvaia_align_load_block.argtypes = [vp, C.c_void_p, C.POINTER(C.c_int64), C.c_int]
        L.uvaia_align_run.argtypes = [vp]
        L.uvaia_align_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_double), pi, C.POINTER(C.c_double)]
        self.ptr = vp()
        self._chk(L.uvaia_align_open(C.byref(self.ptr), ref, len(ref), 0, None))
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        self._chk(L.uvaia_align_load_block(self.ptr, b"".join(seqs), off.ctypes.data_as(C.POINTER(C.c_int64)), len(seqs)))

    def _chk(self, rc):
        if rc:
            raise RuntimeError("parent library: %d %s" % (rc, (self.L.uvaia_align_last_error(self.ptr) or b"").decode()))

    def run(self):
        self._chk(self.L.uvaia_align_run(self.ptr))
        cells, ms = C.c_ulonglong(0), C.c_double(0)
        self._chk(self.L.uvaia_align_stats(self.ptr, C.byref(cells), None, None, C.byref(ms)))
        return cells.value, ms.value

    def close(self):
        self.L.uvaia_align_close(self.ptr)


def library(ref, seqs, rounds, parent_lib):
    out = {}
    parent = ParentAligner(parent_lib, ref, seqs) if parent_lib else None
    with align.Aligner(ref) as al:
        al.load(seqs)
        al.run()                                                # warm-up: the workspace
        if parent:
            parent.run()
        ms = {"parent": [], "off": [], "on": []}
        var_ms, answer, parent_cells = [], {}, None
        for rnd in range(rounds + 1):                           # round 0 warms every kernel and is not counted
            for mode in ("parent", "off", "on"):
                if mode == "parent":
                    if not parent:
                        continue
                    parent_cells, k_ms = parent.run()
                    if rnd:
                        ms[mode].append(k_ms)
                    continue
                al.set_variants(mode == "on")
                al.variants_ms(reset=True)
                al.run()
                st = al.stats()
                if rnd:
                    ms[mode].append(st["kernel_ms"])
                    if mode == "on":
                        var_ms.append(al.variants_ms())
                else:
                    score, rows = al.fetch()
                    answer[mode] = (score.copy(), rows.copy(), st["cells"], st["passes"])
        rec, qc = al.variants()
    if parent:
        parent.close()
    off, on = spread(ms["off"]), spread(ms["on"])
    out["kernel_ms_per_pool"] = {"off": off, "on": on, "on_minus_off_median": round(on["median"] - off["median"], 3)}
    if parent:
        p = spread(ms["parent"])
        out["kernel_ms_per_pool"].update({"parent": p, "parent_spread": round(p["max"] - p["min"], 3), "off_median_not_above_parents_max": off["median"] <= p["max"],
                                          "on_median_not_above_parents_max": on["median"] <= p["max"]})
        out["same_cells_as_parent"] = parent_cells == answer["off"][2]
    out["same_rows_scores_cells_passes"] = bool(np.array_equal(answer["off"][0], answer["on"][0]) and np.array_equal(answer["off"][1], answer["on"][1]) and answer["off"][2:] == answer["on"][2:])
    v = spread(var_ms)
    floor_ms = 2.0 * len(seqs) * (NCHAR + 1) / (read_ceiling() * 1e9) * 1e3
    out["variants_ms_per_pool"] = v
    out["floor"] = {"bytes": 2 * len(seqs) * (NCHAR + 1), "read_GBps": read_ceiling(), "ms": round(floor_ms, 4), "variants_ms_over_floor": round(v["median"] / floor_ms, 2)}
    out["variants_ms_over_aligner_kernel_ms"] = round(v["median"] / on["median"], 5)
    out["records"] = int(rec.size)
    out["substitutions"] = int(qc["substitutions"].sum())
    out["deletion_runs"] = int(qc["deletion_runs"].sum())
    out["deleted_sites"] = int(qc["deleted_sites"].sum())
    # the records of a sample of rows against the numpy restatement; the counts of all rows against the invariant
    rows = answer["on"][1]
    sample = list(range(0, len(seqs), max(1, len(seqs) // 64)))
    at = np.concatenate([[0], np.cumsum(qc["substitutions"].astype(np.int64) + qc["deletion_runs"])])
    ok = True
    for q in sample:
        w_rec, w_qc = AV.restate_row(rows[q].tobytes(), ref)
        ok = ok and AV.records_of(rec[at[q]:at[q + 1]]) == [(q,) + r for r in w_rec] and AV.counts_of(qc[q:q + 1]) == [w_qc]
    out["sample_equals_the_restatement"] = bool(ok)
    out["invariant_holds"] = bool(((qc["matches"] + qc["substitutions"] + qc["deleted_sites"] + qc["unknown_sites"] + qc["other_sites"]) == len(ref)).all())
    return out, qc, answer["on"][0]


def command(d, ref, seqs, qc, score, rounds):
    ref_fa, fa = os.path.join(d, "ref.fa"), os.path.join(d, "queries.fa")
    with open(ref_fa, "wb") as fh:
        fh.write(b">reference\n" + ref + b"\n")
    with open(fa, "wb") as fh:
        for i, s in enumerate(seqs):
            fh.write(b">q_%d\n" % i + s + b"\n")
    exe = os.path.join(ROOT, "bin", "uvaialign")
    cmds = {"plain": [exe, "-r", ref_fa, "-a", "1.0", "--packed", os.path.join(d, "plain.uvdb"), fa],
            "tables": [exe, "-r", ref_fa, "-a", "1.0", "--packed", os.path.join(d, "var.uvdb"), "--variants", os.path.join(d, "var.csv"), "--qc", os.path.join(d, "qc.csv"), fa]}
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
    lines = open(os.path.join(d, "qc.csv"), "rb").read().split(b"\n")[1:-1]
    same = len(lines) == len(seqs)
    for q, ln in enumerate(lines if same else []):
        f = ln.split(b",")
        same = same and f[0] == b"q_%d" % q and int(f[1]) == len(seqs[q]) and int(f[2]) == int(score[q]) and \
            [int(x) for x in f[3:7] + f[9:13]] == [int(qc[q][k]) for k in AV.QC_FIELDS]
    p = spread(wall["plain"])
    out = {"command": "uvaialign -r ref.fa -a 1.0 --packed out.uvdb [--variants var.csv --qc qc.csv] queries.fa", "wall_s": {"plain": p, "tables": spread(wall["tables"])},
           "align_ms": {k: spread(v) for k, v in dev.items()}, "same_database": filecmp.cmp(os.path.join(d, "plain.uvdb"), os.path.join(d, "var.uvdb"), shallow=False),
           "qc_table_is_the_librarys": bool(same), "variants_table_bytes": os.path.getsize(os.path.join(d, "var.csv")), "qc_table_bytes": os.path.getsize(os.path.join(d, "qc.csv"))}
    out["tables_minus_plain_median_s"] = round(out["wall_s"]["tables"]["median"] - p["median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cli-rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--dir", default="/tmp/align_variants")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    ref, seqs = workload(a.queries)
    result = {"queries": len(seqs), "nchar": NCHAR, "rounds": a.rounds, "cli_rounds": a.cli_rounds, "parent_library": bool(a.parent_lib), "cold_cache": "not measured"}
    result["library"], qc, score = library(ref, seqs, a.rounds, a.parent_lib)
    if a.cli_rounds > 0:
        result["command"] = command(a.dir, ref, seqs, qc, score, a.cli_rounds)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
