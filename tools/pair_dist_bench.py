#!/usr/bin/env python3
"""All pairs of the resident database against each other (kernels_pairs.inc) on the GPU box.  Nothing is asserted; the numbers are recorded.
  (a) kernels        generator genomes (host/synth.c, SARS-CoV-2 length) resident in one engine; device time (uvaia_gpu_pairs_ms) of the dense snp
                     kernel at both row-tile heights and of the five-counter kernel over rows [0, --rows) x columns [0, --refs), and of the
                     threshold form (D = 2, upper) over rows [0, --within-rows) x columns [0, --within-refs): one warming round, --rounds
                     counted ones, median and min-max
  (b) against a bound   vector instructions issued = instructions per pair-word x pairs x words / 64 against README's 614 G wave-instructions/s;
                     column-tile bytes requested = row tiles x column tiles x tile bytes against the measured read ceiling (0.89 of 8 TB/s)
  (c) CPU            the oracle's two kernels over all pairs of a --cpu-rows sample on 16 threads
  (d) whole command  `uvaiadist --packed` of the --refs rows to /dev/null and to a file, split by its report
Writes profiles/pair_dist.json and prints it.
Usage: python tools/pair_dist_bench.py [--refs 20000] [--rows 4096] [--within-refs 100000] [--within-rows 8192] [--cpu-rows 2000] [--dir /tmp/pair_dist]"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from uvaia_amd import capi, hostlib  # noqa: E402

NCHAR = 29903
VALU_RATE = 614e9            # wave-instructions/s, README's measured figure
READ_CEILING = 0.89 * 8e12   # bytes/s, the box's read-only ceiling (README)
INSTR = {"snp": 4, "counts": 17}
ROW_TILE = {"snp_32": 32, "snp_64": 64, "counts": 16, "within": 16}


def spread(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "all_ms": [round(x, 3) for x in v]}


def bound(kind, key, n_rows, n_cols, ms):
    words = (NCHAR + 31) // 32
    w4 = (words + 3) // 4
    instr = INSTR[kind] * n_rows * n_cols * w4 * 4 / 64
    tile_bytes = -(-n_rows // ROW_TILE[key]) * -(-n_cols // 64) * w4 * 4096
    t = ms * 1e-3
    return {"pairs": n_rows * n_cols, "pairs_per_s": round(n_rows * n_cols / t), "vector_wave_instructions": int(instr), "fraction_of_valu_rate": round(instr / t / VALU_RATE, 3),
            "column_tile_bytes_requested": int(tile_bytes), "requested_bytes_per_s_over_read_ceiling": round(tile_bytes / t / READ_CEILING, 3)}


def kernels(a, doc):
    import oracle_lib as O
    gen = hostlib.Synth()
    root = bytes(b"ACGT"[s & 3] for s in range(NCHAR))
    n = max(a.refs, a.within_refs)
    with capi.Engine.from_query(O.Query([root], ["q"]), nbest=1, max_pool=64, device=a.device) as eng:
        eng.db_reserve(n)
        t0 = time.perf_counter()
        for first in range(0, n, 4096):
            rows, non_n = gen.generate(first, min(4096, n - first))
            eng.db_append_block(rows, non_n)
        doc["load_s"] = round(time.perf_counter() - t0, 2)
        res = {}
        for key, what, rows_ in (("snp_32", capi.PAIRS_SNP, a.rows), ("snp_64", capi.PAIRS_SNP_ALT, a.rows), ("counts", capi.PAIRS_COUNTS, a.rows // 2)):
            out = np.zeros((rows_, a.refs) + ((5,) if what == capi.PAIRS_COUNTS else ()), dtype=np.int32)
            ms, prep = [], []
            for r in range(a.rounds + 1):
                eng.pairs_ms(reset=True)
                eng.db_pairs(rows=(0, rows_), cols=(0, a.refs), what=what, out=out)
                m = eng.pairs_ms()
                if r:
                    ms.append(m["dense"]); prep.append(m["rows"])
            kind = "counts" if key == "counts" else "snp"
            res[key] = dict(spread(ms), rows=rows_, cols=a.refs, row_operands=spread(prep), **bound(kind, key, rows_, a.refs, statistics.median(ms)))
            res[key]["whole_matrix_ms_scaled"] = round(statistics.median(ms) * a.refs / rows_, 1)
        ms, found = [], 0
        for r in range(a.rounds + 1):
            eng.pairs_ms(reset=True)
            _recs, found = eng.db_pairs_within(2, rows=(0, a.within_rows), cols=(0, a.within_refs), metric=capi.DIST_SNP, upper=True, cap=1 << 22)
            if r:
                ms.append(eng.pairs_ms()["within"])
        computed = sum(min(1024, a.within_rows - rb) * min(8192, a.within_refs - cb) for rb in range(0, a.within_rows, 1024) for cb in range(0, a.within_refs, 8192) if cb + min(8192, a.within_refs - cb) > rb + 1)
        res["within_d2_upper"] = dict(spread(ms), rows=a.within_rows, cols=a.within_refs, found=int(found), pairs_counted_by_the_launches=computed,
                                      fraction_of_valu_rate=round(INSTR["counts"] * computed * 936 / 64 / (statistics.median(ms) * 1e-3) / VALU_RATE, 3))
        doc["kernels"] = res
        best = min(("snp_32", "snp_64"), key=lambda k: res[k]["median_ms"])
        doc["row_tile_heights"] = {"faster": best, "snp_32_median_ms": res["snp_32"]["median_ms"], "snp_64_median_ms": res["snp_64"]["median_ms"]}


def cpu_side(a, doc):
    import oracle_lib as O
    L = O.lib()
    gen = hostlib.Synth()
    rows, _ = gen.generate(0, a.cpu_rows)
    seqs = [rows[i].tobytes() for i in range(a.cpu_rows)]
    idx = (C.c_size_t * NCHAR)(*range(NCHAR))

    def row(i):
        r4, r2 = (C.c_int * 4)(), (C.c_int * 2)()
        for j in range(i + 1, a.cpu_rows):
            L.orc_score_matches_truncated_idx(seqs[i], seqs[j], NCHAR, 2 ** 31 - 1, r4, idx)
            L.orc_score_acgt_and_valid(seqs[i], seqs[j], NCHAR, 2 ** 31 - 1, r2, idx)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(row, range(a.cpu_rows)))
    t = time.perf_counter() - t0
    pairs = a.cpu_rows * (a.cpu_rows - 1) // 2
    doc["cpu_oracle_16_threads"] = {"rows": a.cpu_rows, "pairs": pairs, "seconds": round(t, 2), "pairs_per_s": round(pairs / t)}


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
    res = {}
    for key, target in (("to_dev_null", ["-o", "/dev/null"]), ("to_a_file", ["-o", os.path.join(a.dir, "dist.tsv")])):
        runs = []
        for _ in range(a.command_rounds):
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(ROOT, "bin", "uvaiadist")] + target + ["--packed", db], stderr=subprocess.PIPE, check=True)
            rep = json.loads(re.search(rb"dist report: (\{.*\})", r.stderr).group(1))
            rep["wall_s"] = round(time.perf_counter() - t0, 2)
            runs.append(rep)
        res[key] = runs
    last = res["to_dev_null"][-1]
    res["kernel_share_of_the_command"] = round(last["kernel_ms"] / (last["wall_s"] * 1e3), 3)
    doc["whole_command"] = res
    for f in ("dist.tsv", "refs.uvdb"):
        if os.path.exists(os.path.join(a.dir, f)):
            os.remove(os.path.join(a.dir, f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--within-refs", type=int, default=100000)
    ap.add_argument("--within-rows", type=int, default=8192)
    ap.add_argument("--cpu-rows", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--command-rounds", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dir", default="/tmp/pair_dist")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_dist.json"))
    a = ap.parse_args()
    doc = {"nchar": NCHAR, "refs": a.refs, "rounds": a.rounds, "valu_rate_wave_instructions_per_s": VALU_RATE, "read_ceiling_bytes_per_s": READ_CEILING,
           "instructions_per_pair_word": INSTR, "not_measured": []}
    for name, f in (("kernels", kernels), ("cpu_oracle_16_threads", cpu_side), ("whole_command", whole_command)):
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
