#!/usr/bin/env python3
"""`uvaiaball --packed` against `uvaiaball -r` on generator references, and the pieces on their own (on the GPU box).
Writes one JSON document; every number carries the command or call that produced it.

  whole command   bin/uvaiaball -r refs.fa  vs  bin/uvaiaball --packed refs.uvdb, at a small and a large radius, with the progress lines
  unpack alone    uvdb_unpack_reference over the kept list (1 thread, 16 threads) vs uvaia_gpu_unpack_rows (copy-back included)
  search alone    uvaia_gpu_ball_kernel_ms of packed batches vs text batches of the same references, three repeats

Usage: python tools/ball_packed_bench.py [--refs 100000] [--queries 100] [--radii 2,4000] [--dir /tmp/ballpacked] [--out profiles/ball_packed.json] [--xz]
       python tools/ball_packed_bench.py --unpack-only ...     (the unpack calls alone, e.g. under rocprofv3 --kernel-trace --stats)"""
import argparse
import ctypes as C
import json
import lzma
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uvaia_amd import capi, hostlib  # noqa: E402

BALL, PACK = os.path.join(ROOT, "bin", "uvaiaball"), os.path.join(ROOT, "bin", "uvaiapack")


def run(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    err = r.stderr.decode(errors="replace")
    if r.returncode:
        sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), err[-3000:]))
        sys.exit(1)
    return {"command": " ".join(os.path.relpath(c, ROOT) if c.startswith(ROOT) else c for c in cmd), "wall_s": round(dt, 3),
            "progress_lines": [l for l in err.splitlines() if "secs" in l or "seconds" in l or "Saved" in l]}


class Uvdb:
    """the packed file as the host library maps it (uvaia_amd/csrc/host/uvdb.h)"""

    def __init__(self, path):
        self.L = hostlib.load_library()
        self.L.uvdb_open.restype = C.c_void_p
        self.L.uvdb_open.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
        self.L.uvdb_unpack_reference.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        self.L.uvdb_unpack_reference.restype = None
        err = C.create_string_buffer(512)
        self.r = self.L.uvdb_open(path.encode(), err, 512)
        if not self.r:
            raise RuntimeError(err.value.decode())
        hdr = np.fromfile(path, dtype=np.uint8, count=128)
        self.nchar, self.W4 = int(hdr[12:16].view(np.uint32)[0]), int(hdr[16:20].view(np.uint32)[0])
        self.n_ref, self.n_tiles, self.tile_bytes = (int(x) for x in hdr[24:48].view(np.uint64))
        off_planes = int(hdr[56:64].view(np.uint64)[0])
        self.planes = np.memmap(path, dtype=np.uint8, mode="r", offset=off_planes, shape=(self.n_tiles, self.tile_bytes))

    def unpack_list(self, index, out):
        for k, i in enumerate(index):
            self.L.uvdb_unpack_reference(self.r, int(i), out[k].ctypes.data)


def median3(f):
    v = sorted(f() for _ in range(3))
    return round(v[1], 4), [round(x, 4) for x in v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--radii", default="2,4000")
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--dir", default="/tmp/ballpacked")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ball_packed.json"))
    ap.add_argument("--xz", action="store_true", help="also time the text path on an xz-compressed copy of the references")
    ap.add_argument("--unpack-only", action="store_true")
    ap.add_argument("--skip-commands", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    radii = [int(x) for x in a.radii.split(",")]
    gen = hostlib.Synth()
    ref_fa, q_fa, db = (os.path.join(a.dir, x) for x in ("refs.fa", "query.fa", "refs.uvdb"))
    if not os.path.exists(db):
        with open(ref_fa, "wb") as fh:
            for first in range(0, a.refs, 2048):
                rows, _ = gen.generate(first, min(2048, a.refs - first))
                for i in range(rows.shape[0]):
                    fh.write(b">ref_%d\n" % (first + i) + rows[i].tobytes() + b"\n")
    qrows, _ = gen.generate(10_000_000, a.queries)
    qs = [qrows[i].tobytes() for i in range(a.queries)]
    with open(q_fa, "wb") as fh:
        for i, s in enumerate(qs):
            fh.write(b">q_%d\n" % i + s + b"\n")
    doc = {"refs": a.refs, "queries": a.queries, "nchar": gen.nchar, "chunk": a.chunk, "radii": radii, "commands": {}, "unpack": {}, "search": {}}
    if not os.path.exists(db):
        doc["uvaiapack"] = run([PACK, "-o", db, ref_fa])
    doc["uvdb_bytes"] = os.path.getsize(db)

    # ---- whole commands
    if not a.unpack_only and not a.skip_commands:
        if a.xz:
            with open(ref_fa, "rb") as src, lzma.open(ref_fa + ".xz", "wb", preset=1) as dst:
                for block in iter(lambda: src.read(1 << 24), b""):
                    dst.write(block)
        for d in radii:
            entry = {}
            run([BALL, "--packed", db, q_fa, "-d", str(d), "-o", os.path.join(a.dir, "warm")])          # page cache and device warm
            entry["packed"] = run([BALL, "--packed", db, q_fa, "-d", str(d), "-p", str(a.chunk), "-o", os.path.join(a.dir, "p%d" % d)])
            entry["text"] = run([BALL, "-r", ref_fa, q_fa, "-d", str(d), "-p", str(a.chunk), "-o", os.path.join(a.dir, "t%d" % d)])
            if a.xz:
                entry["text_xz_input"] = run([BALL, "-r", ref_fa + ".xz", q_fa, "-d", str(d), "-p", str(a.chunk), "-o", os.path.join(a.dir, "x%d" % d)])
            entry["same_dump"] = open(os.path.join(a.dir, "p%d.aln.xz" % d), "rb").read() == open(os.path.join(a.dir, "t%d.aln.xz" % d), "rb").read()
            doc["commands"]["d=%d" % d] = entry

    # ---- the pieces, through the C ABI: the first chunk of the file
    u = Uvdb(db)
    n = min(a.chunk, u.n_ref)
    pq = hostlib.PreparedQuery(qs, ["q_%d" % i for i in range(len(qs))], dist=1, is_ball=True)
    pitch = (u.nchar + 15) // 16 * 16
    with pq.open_engine(nbest=2, max_pool=n) as eng:
        tiles = np.ascontiguousarray(u.planes[:(n + 63) // 64])
        for d in radii:
            md = eng.ball_packed(tiles, n, d + 1)
            kept = np.nonzero(md <= d)[0].astype(np.int32)
            rows = np.zeros((max(len(kept), 1), pitch), dtype=np.uint8)
            idx = kept.ctypes.data_as(C.POINTER(C.c_int))

            def device():
                t0 = time.perf_counter()
                eng._chk(eng.L.uvaia_gpu_unpack_rows(eng.ctx, idx, len(kept), rows.ctypes.data, pitch))
                return time.perf_counter() - t0

            device()                                                                                    # warm-up: staging buffers, code object
            dev, dev_all = median3(device)
            entry = {"kept": int(len(kept)), "of": int(n), "kept_share": round(len(kept) / n, 4),
                     "uvaia_gpu_unpack_rows_s": dev, "uvaia_gpu_unpack_rows_repeats": dev_all,
                     "call": "Engine.ball_packed(first chunk, d + 1) then uvaia_gpu_unpack_rows(kept, pageable rows of %d bytes), median of 3 after a warm-up" % pitch,
                     "bytes_moved_device": int(len(kept)) * (u.W4 * 4 * 16 + u.nchar)}
            if not a.unpack_only:
                out = np.zeros((max(len(kept), 1), u.nchar + 1), dtype=np.uint8)

                def host1():
                    t0 = time.perf_counter()
                    u.unpack_list(kept, out)
                    return time.perf_counter() - t0

                def host16():
                    t0 = time.perf_counter()
                    parts = np.array_split(np.arange(len(kept)), 16)
                    with ThreadPoolExecutor(16) as ex:
                        list(ex.map(lambda p: u.unpack_list(kept[p], out[p[0]:p[0] + len(p)]) if len(p) else None, parts))
                    return time.perf_counter() - t0

                few = kept[:2000]                                                                       # one thread: a sample, scaled
                t0 = time.perf_counter()
                u.unpack_list(few, out)
                entry["uvdb_unpack_reference_1_thread_s"] = round((time.perf_counter() - t0) * len(kept) / max(len(few), 1), 4)
                entry["uvdb_unpack_reference_1_thread_call"] = "uvdb_unpack_reference over the first %d kept references, scaled to all of them" % len(few)
                entry["uvdb_unpack_reference_16_threads_s"], entry["uvdb_unpack_reference_16_threads_repeats"] = median3(host16)
                entry["uvdb_unpack_reference_16_threads_call"] = "16 threads (the calls release the interpreter lock), a sixteenth of the kept list each"
                same = all(out[k, :u.nchar].tobytes().replace(b"-", b"N") == rows[k, :u.nchar].tobytes() for k in range(0, len(kept), max(1, len(kept) // 50)))
                entry["same_text_up_to_exceptions"] = bool(same)
            doc["unpack"]["d=%d" % d] = entry

        # ---- the search itself: packed batches against text batches of the same references
        if not a.unpack_only:
            m = min(n, 8192)
            text_rows, _ = gen.generate(0, m)
            text = [text_rows[i].tobytes() for i in range(m)]
            d = radii[0]
            for tag, call in (("packed", lambda: eng.ball_packed(tiles, m, d + 1)), ("text", lambda: eng.ball(text, d + 1))):
                call()
                reps = []
                for _ in range(3):
                    eng.ball_kernel_ms(reset=True)
                    call()
                    reps.append([round(x, 4) for x in eng.ball_kernel_ms(reset=True)])
                doc["search"][tag] = {"ball_kernel_ms_consensus_gather_scan": reps, "references": m, "radius": d + 1,
                                      "call": "Engine.%s over the first %d references, three repeats after a warm-up" % ("ball_packed" if tag == "packed" else "ball", m)}
    if a.unpack_only:
        print(json.dumps(doc["unpack"]))
        return
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
