#!/usr/bin/env python3
"""`uvaiaclust --packed` against `uvaiaclust` on text, on the bundled alignment and on the synthetic family rows of tools/cluster_bench.py
(on the GPU box).  Writes one JSON document; every number carries the command or call that produced it.

  whole commands   bin/uvaiaclust seqs.fa  vs  bin/uvaiaclust --packed seqs.uvdb: alternating, three repeats, medians; the time up to the
                   end of the last push with the prep and queue kernels taken off (= reading, parsing, copying, decoding: the ingest), and
                   whether the two pairs of output files are identical
  decode kernel    clust_unpack_tiles_kernel per chunk of 4 096 references through the C ABI (uvaia_clust_unpack_ms), and the bytes per
                   second it reaches: tile_bytes / 64 read and one row pitch written per reference, against the 8 TB/s peak
  routes           uvaiaclust + uvaiapack of its <prefix>.aln.xz  vs  one uvaiaclust --packed --packed-out

Usage: python tools/cluster_packed_bench.py [--synthetic 100000] [--dir /tmp/clustpacked] [--out profiles/cluster_packed.json]
       python tools/cluster_packed_bench.py --kernel-only ...   (the pushes alone, e.g. under rocprofv3 --kernel-trace --stats)"""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_lib as CL  # noqa: E402
import fixtures as F  # noqa: E402
from uvaia_amd import cluster  # noqa: E402

CLUST, PACK = os.path.join(ROOT, "bin", "uvaiaclust"), os.path.join(ROOT, "bin", "uvaiapack")
CHUNK = 4096
PEAK = 8e12


def run(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    err = r.stderr.decode(errors="replace")
    if r.returncode:
        sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), err[-3000:]))
        sys.exit(1)
    out = {"command": " ".join(os.path.relpath(c, ROOT) if c.startswith(ROOT) else c for c in cmd), "wall_s": round(dt, 3)}
    m = re.findall(r"Finished reading file .* in ([0-9.]+) secs", err)
    k = re.search(r"prep ([0-9.]+) ms, queues ([0-9.]+) ms, merge ([0-9.]+) ms, decode ([0-9.]+) ms, overlay ([0-9.]+) ms", err)
    if m and k:
        prep, queue, merge, decode, overlay = (float(x) for x in k.groups())
        out.update(read_s=float(m[-1]), kernels_ms={"prep": prep, "queue": queue, "merge": merge, "decode": decode, "overlay": overlay},
                   ingest_s=round(float(m[-1]) - (prep + queue) / 1000., 3))
    return out


def write_fasta(path, names, seqs):
    with open(path, "wb") as fh:
        for n, s in zip(names, seqs):
            fh.write(b">" + n.encode() + b"\n" + s + b"\n")


def same_files(a, b):
    return all(lzma.open(a + x, "rb").read() == lzma.open(b + x, "rb").read() for x in (".csv.xz", ".aln.xz"))


def median_of(runs, key):
    return round(statistics.median(r[key] for r in runs), 3)


def commands(d, tag, args):
    fa, db = os.path.join(d, tag + ".fa"), os.path.join(d, tag + ".uvdb")
    doc = {"uvaiapack": run([PACK, "-A", "1", "-o", db, fa])}
    text, packed = [], []
    run([CLUST] + args + ["--packed", db, "-o", os.path.join(d, tag + "_warm")])                        # page cache and device warm
    for _ in range(3):                                                                                  # alternating
        text.append(run([CLUST] + args + ["-o", os.path.join(d, tag + "_text"), fa]))
        packed.append(run([CLUST] + args + ["--packed", db, "-o", os.path.join(d, tag + "_packed")]))
    doc["text"], doc["packed"] = text, packed
    doc["median"] = {k: {"wall_s": median_of(v, "wall_s"), "ingest_s": median_of(v, "ingest_s")} for k, v in (("text", text), ("packed", packed))}
    doc["ingest_definition"] = "seconds up to the end of the last push (the command's 'Finished reading file' line) minus its prep and queue kernel time"
    doc["packed_ingest_not_longer_than_text"] = doc["median"]["packed"]["ingest_s"] <= doc["median"]["text"]["ingest_s"]
    doc["same_output_files"] = same_files(os.path.join(d, tag + "_text"), os.path.join(d, tag + "_packed"))
    # the routes to a deduplicated packed database
    three = [run([CLUST] + args + ["-o", os.path.join(d, tag + "_r3"), fa]), run([PACK, "-A", "1", "-o", os.path.join(d, tag + "_r3.uvdb"), os.path.join(d, tag + "_r3.aln.xz")])]
    one = run([CLUST] + args + ["--packed", db, "--packed-out", os.path.join(d, tag + "_r1.uvdb"), "-o", os.path.join(d, tag + "_r1")])
    doc["routes"] = {"uvaiaclust_then_uvaiapack": three, "uvaiaclust_then_uvaiapack_wall_s": round(sum(x["wall_s"] for x in three), 3), "uvaiaclust_packed_packed_out": one,
                     "note": "the text route starts from text and the packed route from the database `uvaialign --packed` would have written; packing the input is the line uvaiapack above",
                     "same_database": open(os.path.join(d, tag + "_r3.uvdb"), "rb").read() == open(os.path.join(d, tag + "_r1.uvdb"), "rb").read()}
    return doc


def kernel(db, dist, n_queues):
    """the pushes of a database through the C ABI, chunk by chunk: decode and overlay time of every chunk"""
    hdr = np.fromfile(db, dtype=np.uint8, count=128)
    nchar = int(hdr[12:16].view(np.uint32)[0])
    n_ref, n_tiles, tile_bytes = (int(x) for x in hdr[24:48].view(np.uint64))
    off = {k: int(hdr[56 + 8 * i:64 + 8 * i].view(np.uint64)[0]) for i, k in enumerate(("planes", "nonn", "side", "name_idx", "names", "exc_idx", "exc", "file"))}
    planes = np.memmap(db, dtype=np.uint8, mode="r", offset=off["planes"], shape=(n_tiles, tile_bytes))
    exc_idx = np.fromfile(db, dtype=np.uint64, count=n_ref + 1, offset=off["exc_idx"])
    exc = np.fromfile(db, dtype=np.uint32, offset=off["exc"]).reshape(-1, 2)
    ref = b"ACGT" * (nchar // 4) + b"ACGT"[:nchar % 4]
    chunks = []
    with cluster.Clusterer(ref, dist=dist, n_queues=n_queues) as c:
        last = {"decode_ms": 0., "overlay_ms": 0.}
        for a in range(0, n_ref, CHUNK):
            n = min(CHUNK, n_ref - a)
            c.push_packed(np.ascontiguousarray(planes[a // 64:(a + n + 63) // 64]), n, exc_idx[a:a + n + 1], exc, (np.arange(a, a + n) % n_queues).astype(np.int32))
            ms = c.unpack_ms()
            chunks.append({"references": n, "decode_ms": round(ms["decode_ms"] - last["decode_ms"], 4), "overlay_ms": round(ms["overlay_ms"] - last["overlay_ms"], 4),
                           "records": int(exc_idx[a + n] - exc_idx[a])})
            last = ms
    pitch = (nchar + 63) // 64 * 64
    full = [k for k in chunks if k["references"] == CHUNK] or chunks
    per = statistics.median(k["decode_ms"] for k in full[1:] or full)
    moved = full[0]["references"] * (tile_bytes // 64 + pitch)
    return {"nchar": nchar, "references": n_ref, "chunk": CHUNK, "bytes_per_reference": {"read": tile_bytes // 64, "written": pitch}, "chunks": chunks,
            "decode_ms_per_full_chunk_median": round(per, 4), "decode_bytes_per_s": round(moved / (per / 1000.), 0), "share_of_8_TB_s": round(moved / (per / 1000.) / PEAK, 4),
            "call": "Clusterer.push_packed over the database in chunks of %d, uvaia_clust_unpack_ms after each; the first chunk (code object load) left out of the median" % CHUNK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", type=int, default=100000)
    ap.add_argument("--dir", default="/tmp/clustpacked")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_packed.json"))
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    names, seqs = F.load_bundled()
    sets = {"bundled": (names, seqs, ["-d", "1", "-p", "64"], 1)}
    if a.synthetic:
        fam = CL.families(a.synthetic, a.synthetic // 13, 20261017)
        sets["synthetic_families"] = (["fam_%d" % i for i in range(len(fam))], fam, ["-d", "3", "-p", "64"], 3)
    doc = {}
    for tag, (nm, sq, args, dist) in sets.items():
        fa, db = os.path.join(a.dir, tag + ".fa"), os.path.join(a.dir, tag + ".uvdb")
        if not os.path.exists(fa):
            write_fasta(fa, nm, sq)
        if a.kernel_only:
            if not os.path.exists(db):
                run([PACK, "-A", "1", "-o", db, fa])
            doc[tag] = {"decode_kernel": kernel(db, dist, 64)}
            continue
        doc[tag] = {"sequences": len(sq), "nchar": len(sq[0]), "arguments": " ".join(args)}
        doc[tag].update(commands(a.dir, tag, args))
        doc[tag]["decode_kernel"] = kernel(db, dist, 64)
    if a.kernel_only:
        print(json.dumps(doc))
        return
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({t: {"median": v["median"], "same_output_files": v["same_output_files"], "routes_same_database": v["routes"]["same_database"],
                          "decode_ms_per_chunk": v["decode_kernel"]["decode_ms_per_full_chunk_median"], "share_of_8_TB_s": v["decode_kernel"]["share_of_8_TB_s"]}
                      for t, v in doc.items()}))


if __name__ == "__main__":
    main()
