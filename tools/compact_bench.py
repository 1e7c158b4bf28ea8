#!/usr/bin/env python3
"""The compact packed database (`uvaiapack --compact`, version 2 of uvaia_amd/csrc/host/uvdb.h) on the GPU box, against the dense file of the
same references.  Nothing is asserted but equal outputs; every figure is reported as measured.
  sizes     dense and compact file size, bytes per reference of heads and of literals, for the bundled alignment and for generator genomes
            (tools/ingest_bench.py's generator: SARS-CoV-2 length, its default divergence and N content)
  commands  `uvaia --packed` on the dense and on the compact file, alternating in one session, the first round (which warms the page
            cache of both files) not counted: the "Loaded ... in" time and the wall time, resident and with --window at a quarter of
            the database (--window-report's upload and free-memory figures); with --parent-bin the parent commit's `uvaia` runs on the dense
            file in the same rounds: the yardstick
  device    time of expand_tiles_kernel and of the side-row pass per million references (HIP events around both, uvaia_gpu_compact_ms),
            and the time uvdb_open takes on either file (the compact one: every head is checked)
Writes profiles/compact_db.json and prints it.
Usage: python tools/compact_bench.py [--refs 100000] [--queries 1000] [--dir /tmp/compact_bench] [--parent-bin <dir with the parent's uvaia>]"""
import argparse
import ctypes as C
import json
import lzma
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


def sections(path):
    """sizes of a packed database's sections from its header"""
    with open(path, "rb") as fh:
        h = np.frombuffer(fh.read(136), dtype=np.uint8)
    u32, u64 = (lambda o: int(h[o:o + 4].view(np.uint32)[0])), (lambda o: int(h[o:o + 8].view(np.uint64)[0]))
    out = {"version": u32(8), "nchar": u32(12), "n_ref": u64(24), "n_tiles": u64(32), "file_bytes": os.path.getsize(path)}
    if out["version"] == 2:
        lanes = out["n_tiles"] * 64
        off_hidx, off_heads, off_lidx = u64(72), u64(120), u64(128)
        with open(path, "rb") as fh:
            fh.seek(off_hidx + 8 * lanes); n_heads = int(np.frombuffer(fh.read(8), dtype=np.uint64)[0])
            fh.seek(off_lidx + 8 * lanes); n_lits = int(np.frombuffer(fh.read(8), dtype=np.uint64)[0])
        out.update({"heads": n_heads, "literal_words": n_lits, "off_base": u64(56), "off_nonn": u64(64), "off_head_idx": off_hidx, "off_heads": off_heads,
                    "off_lit_idx": off_lidx, "off_lits": (off_lidx + (lanes + 1) * 8 + 63) // 64 * 64})
    return out


def size_report(dense, compact):
    d, c = sections(dense), sections(compact)
    n = max(c["n_ref"], 1)
    return {"n_ref": c["n_ref"], "nchar": c["nchar"], "dense_bytes": d["file_bytes"], "compact_bytes": c["file_bytes"],
            "ratio_dense_over_compact": round(d["file_bytes"] / c["file_bytes"], 2),
            "dense_bytes_per_ref": round(d["file_bytes"] / n, 1), "compact_bytes_per_ref": round(c["file_bytes"] / n, 1),
            "heads_per_ref": round(c["heads"] / n, 2), "head_bytes_per_ref": round(4 * c["heads"] / n, 1),
            "literal_words_per_ref": round(c["literal_words"] / n, 2), "literal_bytes_per_ref": round(16 * c["literal_words"] / n, 1),
            "index_bytes_per_ref": 16, "names_runs_counts_bytes_per_ref": round((c["file_bytes"] - 4 * c["heads"] - 16 * c["literal_words"]) / n - 16, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dir", default="/tmp/compact_bench")
    ap.add_argument("--pool", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-bin", default=None, help="directory with the parent commit's uvaia: run on the dense file in the same rounds")
    ap.add_argument("--skip-bundled", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_db.json"))
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    gen = hostlib.Synth()
    uv, pk = os.path.join(ROOT, "bin", "uvaia"), os.path.join(ROOT, "bin", "uvaiapack")

    def run(cmd):
        sys.stderr.write("running %s\n" % " ".join(cmd[:1] + cmd[-3:])); sys.stderr.flush()
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        wall = time.perf_counter() - t0
        err = r.stderr.decode(errors="replace")
        if r.returncode:
            sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), err[-3000:]))
            sys.exit(1)
        return wall, err

    result = {"refs": a.refs, "queries": a.queries, "pool": a.pool, "repeats": a.repeats, "sizes": {}}
    # ---- sizes: the bundled alignment
    bundled = os.path.join(ROOT, "tests", "golden", "03.unique_acgt.aln.xz")
    if not a.skip_bundled:
        bd, bc = os.path.join(a.dir, "bundled_dense.uvdb"), os.path.join(a.dir, "bundled_compact.uvdb")
        t_d, _ = run([pk, "-A", "0.999", "-o", bd, bundled])
        t_c, _ = run([pk, "-A", "0.999", "--compact", "-o", bc, bundled])
        result["sizes"]["bundled_alignment"] = dict(size_report(bd, bc), pack_dense_s=round(t_d, 2), pack_compact_s=round(t_c, 2))
    # ---- the generator's genomes
    fa, dense, compact = os.path.join(a.dir, "refs.fa"), os.path.join(a.dir, "dense.uvdb"), os.path.join(a.dir, "compact.uvdb")
    with open(fa, "wb") as fh:
        for first in range(0, a.refs, 2048):
            rows, _ = gen.generate(first, min(2048, a.refs - first))
            for i in range(rows.shape[0]):
                fh.write(b">ref_%d\n" % (first + i) + rows[i].tobytes() + b"\n")
    t_d, _ = run([pk, "-o", dense, fa])
    t_c, _ = run([pk, "--compact", "-o", compact, fa])
    os.remove(fa)
    result["sizes"]["generator"] = dict(size_report(dense, compact), pack_dense_s=round(t_d, 2), pack_compact_s=round(t_c, 2))
    q_fa = os.path.join(a.dir, "query.fa")
    with open(q_fa, "wb") as fh:
        rows, _ = gen.generate(10_000_000, a.queries)
        for i in range(rows.shape[0]):
            fh.write(b">q_%d\n" % i + rows[i].tobytes() + b"\n")

    # ---- whole commands, alternating; round 0 warms the page cache of both files and is not counted
    window = -(-a.refs // 4)
    kinds = [("dense", uv, dense), ("compact", uv, compact)]
    if a.parent_bin:
        kinds.insert(0, ("parent_dense", os.path.join(a.parent_bin, "uvaia"), dense))
    modes = {"resident": ["--window-report"], "window": ["--window", str(window), "--window-report"]}
    runs = {m: {k: {"wall_s": [], "loaded_s": [], "report": []} for k, _, _ in kinds} for m in modes}
    for rep in range(a.repeats + 1):
        for mode, extra in modes.items():
            for kind, exe, db in kinds:
                wall, err = run([exe, q_fa, "-p", str(a.pool), "-n", "100", "-o", os.path.join(a.dir, "out_%s_%s" % (mode, kind)), "--packed", db] + extra)
                if not rep:
                    continue
                e = runs[mode][kind]
                e["wall_s"].append(round(wall, 3))
                m = re.search(r"Loaded \d+ packed sequences from .* in ([0-9.]+) secs", err)
                e["loaded_s"].append(float(m.group(1)) if m else None)
                m = re.search(r"window report: (\{.*\})", err)
                e["report"].append(json.loads(m.group(1)) if m else None)
    result["commands"] = {}
    for mode in modes:
        ref_kind = kinds[0][0]
        want = [lzma.open(os.path.join(a.dir, "out_%s_%s%s" % (mode, ref_kind, s)), "rb").read() for s in (".csv.xz", ".aln.xz")]
        result["commands"][mode] = {}
        for kind, _, _ in kinds:
            e = runs[mode][kind]
            got = [lzma.open(os.path.join(a.dir, "out_%s_%s%s" % (mode, kind, s)), "rb").read() for s in (".csv.xz", ".aln.xz")]
            rep = [r for r in e["report"] if r]
            entry = {"wall_median_s": round(statistics.median(e["wall_s"]), 3), "wall_all_s": e["wall_s"],
                     "loaded_median_s": round(statistics.median(e["loaded_s"]), 3) if all(x is not None for x in e["loaded_s"]) else None, "loaded_all_s": e["loaded_s"],
                     "outputs_equal_%s" % ref_kind: got == want}
            if rep:
                entry["free_before"] = [r["free_before"] for r in rep]
                entry["free_after"] = [r["free_after"] for r in rep]
                if "upload_ms" in rep[0]:
                    entry["upload_ms"] = [r["upload_ms"] for r in rep]
                    entry["upload_hidden_share"] = [r["upload_hidden_share"] for r in rep]
                    entry["select_ms"] = [r["select_ms"] for r in rep]
                    entry["derive_ms"] = [r["derive_ms"] for r in rep]
            result["commands"][mode][kind] = entry
    result["window"] = window

    # ---- uvdb_open: the whole validation (the compact file: every index entry and head)
    L = hostlib.load_library()
    L.uvdb_open.restype = C.c_void_p
    L.uvdb_open.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.uvdb_close_reader.argtypes = [C.c_void_p]
    L.uvdb_close_reader.restype = None
    opens = {}
    for kind, path in (("dense", dense), ("compact", compact)):
        ts = []
        for _ in range(a.repeats + 1):
            err = C.create_string_buffer(512)
            t0 = time.perf_counter()
            r = L.uvdb_open(path.encode(), err, 512)
            ts.append(time.perf_counter() - t0)
            assert r, err.value
            L.uvdb_close_reader(r)
        opens[kind] = {"uvdb_open_median_ms": round(1e3 * statistics.median(ts[1:]), 2), "all_ms": [round(1e3 * t, 2) for t in ts[1:]]}
    result["uvdb_open"] = dict(opens, threads=os.cpu_count() if not os.environ.get("OMP_NUM_THREADS") else int(os.environ["OMP_NUM_THREADS"]))

    # ---- device time of the expansion, chunks of 256 tiles as the resident load stages them
    s = sections(compact)
    lanes = s["n_tiles"] * 64
    raw = np.memmap(compact, dtype=np.uint8, mode="r")
    view = lambda off, n, dt: np.frombuffer(raw, dtype=dt, count=n, offset=off)
    base = view(s["off_base"], (s["nchar"] + 127) // 128 * 16, np.uint32)
    hidx, lidx = view(s["off_head_idx"], lanes + 1, np.uint64), view(s["off_lit_idx"], lanes + 1, np.uint64)
    heads, lits, non_n = view(s["off_heads"], s["heads"], np.uint32), view(s["off_lits"], s["literal_words"] * 4, np.uint32), view(s["off_nonn"], lanes, np.int32)
    qrows, _ = gen.generate(10_000_000, 8)
    q = hostlib.PreparedQuery([qrows[i].tobytes() for i in range(8)], ["q%d" % i for i in range(8)])
    chunk = 256
    with q.open_engine(nbest=4, max_pool=4096) as eng:
        eng.db_stage_reserve(chunk)
        device = []
        for rep in range(a.repeats + 1):
            eng.compact_ms(reset=True)
            t0 = time.perf_counter()
            for t in range(0, s["n_tiles"], chunk):
                nt = min(chunk, s["n_tiles"] - t)
                eng.db_stage_compact_at((t // chunk) & 1, 0, base, hidx[t * 64:(t + nt) * 64 + 1], heads, lidx[t * 64:(t + nt) * 64 + 1], lits, non_n[t * 64:(t + nt) * 64], nt)
            ms = eng.compact_ms()
            device.append((ms[0], ms[1], 1e3 * (time.perf_counter() - t0)))
        device = device[1:]
    per_m = 1e6 / max(lanes, 1)
    result["device"] = {"chunk_tiles": chunk, "lanes": lanes,
                        "expand_tiles_kernel_ms": [round(d[0], 3) for d in device], "side_rows_staged_kernel_ms": [round(d[1], 3) for d in device],
                        "stage_calls_wall_ms": [round(d[2], 1) for d in device],
                        "expand_ms_per_million_refs": round(statistics.median(d[0] for d in device) * per_m, 2),
                        "side_rows_ms_per_million_refs": round(statistics.median(d[1] for d in device) * per_m, 2),
                        "dense_plane_bytes_written_per_ref": (s["nchar"] + 127) // 128 * 64}
    result["note"] = ("wall clock of the whole commands (query preparation, engine start-up, xz output included); page cache WARM for both files (round 0 of "
                      "the alternation reads them and is not counted); loaded_s is the command's own 'Loaded ... in' figure, which in window mode covers no "
                      "upload (the windows are staged during the search: see upload_ms); parent_dense is the parent commit's uvaia on the dense file in the same "
                      "rounds, where --parent-bin was given; stage_calls_wall_ms covers the copies from the mapping and the kernels of all chunks, queued back to back")
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
