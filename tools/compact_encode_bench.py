#!/usr/bin/env python3
"""The compact packed database written from device memory (kernels_encode.inc) on the GPU box, against the parent commit's commands.  One
command, one warming round, then `--repeats` counted rounds with the parent's and this tree's commands alternating; medians and min-max
spreads are reported, outputs are compared byte for byte at the sizes timed.  Nothing is asserted but equal files.
  (a) whole commands   `uvaiapack --compact` of --refs generator genomes (host/synth.c, SARS-CoV-2 length), parent against new;
                       `uvaialign --packed --compact` of --align-seqs unaligned genomes against the parent's `uvaialign --packed` +
                       `uvaiapack --merge --compact`; `uvaiaclust --packed-out --compact` of the first --clust-refs references against the
                       parent's `uvaiaclust --packed-out` + `uvaiapack --merge --compact`
  (b) per batch        of 4 096 references resident in one engine: device time of count + prefix and of emit (uvaia_gpu_encode_ms), wall time
                       of the new route (encode, records, uvdb_add_tiles_encoded) and of the parent's route for the same tiles, a host clock
                       around synchronised calls: uvaia_gpu_db_export + the host encoder (uvdb_add_tiles of a compact writer whose base is fixed)
  (c) bytes            copied to the host per reference, from the indices, against the dense tile and side row
The page cache is warm in every counted round (a cold one is not measured), and nothing is measured at 10 M rows.
Writes profiles/compact_encode.json and prints it.
Usage: python tools/compact_encode_bench.py --parent-bin <parent checkout>/bin [--refs 100000] [--align-seqs 100000] [--clust-refs 12000] [--dir /tmp/compact_encode]"""
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
import bench  # noqa: E402
from uvaia_amd import capi, hostlib  # noqa: E402

BATCH = 4096
DENSE_BYTES_PER_REF = lambda nchar: ((nchar + 31) // 32 + 3) // 4 * 4 * 4 * 4 + 256 + 4      # tile share, side row, valid-site count


def run(cmd):
    sys.stderr.write("running %s\n" % " ".join(os.path.basename(c) if os.sep in c else c for c in cmd)); sys.stderr.flush()
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    err = r.stderr.decode(errors="replace")
    if r.returncode:
        sys.stderr.write("FAILED (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), err[-3000:]))
        sys.exit(1)
    return wall, err


def same(a, b):
    return subprocess.run(["cmp", "-s", a, b]).returncode == 0


def summary(walls):
    return {"median_s": round(statistics.median(walls), 3), "min_s": round(min(walls), 3), "max_s": round(max(walls), 3), "spread_s": round(max(walls) - min(walls), 3), "all_s": [round(w, 3) for w in walls]}


def alternate(ways, repeats):
    """ways: {name: callable -> wall seconds}; one warming round, then `repeats` counted rounds, the ways alternating within a round"""
    walls = {k: [] for k in ways}
    for rep in range(repeats + 1):
        for k, f in ways.items():
            w = f()
            if rep:
                walls[k].append(w)
    return {k: summary(v) for k, v in walls.items()}


def routes(err):
    m = re.search(r"[Cc]ompact tiles: (\d+) encoded on the device.*?(\d+) on the host", err)
    return {"device": int(m.group(1)), "host": int(m.group(2))} if m else None


def verdict(parent, new):
    """the bar of the issue: the new median may not be worse than the parent's by more than the parent's own min-max spread"""
    return {"new_minus_parent_median_s": round(new["median_s"] - parent["median_s"], 3), "parent_spread_s": parent["spread_s"],
            "within_the_bar": bool(new["median_s"] - parent["median_s"] <= parent["spread_s"])}


def per_batch(dense_path, n_batches, device):
    """(b) and (c): batches of 4 096 references of the dense file through one engine and one compact writer"""
    import compact_lib as CL
    import packed_lib as PL
    L = CL._lib()
    L.uvdb_compact_base.restype = C.c_void_p
    L.uvdb_compact_base.argtypes = [C.c_void_p]
    L.uvdb_add_tiles_encoded.restype = C.c_int
    L.uvdb_add_tiles_encoded.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
    L.uvdb_add_reference_runs.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
    h = np.fromfile(dense_path, dtype=np.uint8, count=136)
    u32, u64 = (lambda o: int(h[o:o + 4].view(np.uint32)[0])), (lambda o: int(h[o:o + 8].view(np.uint64)[0]))
    nchar, n_ref, n_tiles, tb, off_planes, off_nonn, off_side = u32(12), u64(24), u64(32), u64(40), u64(56), u64(64), u64(72)
    mm = np.memmap(dense_path, dtype=np.uint8, mode="r")
    bt = BATCH // 64
    n_batches = min(n_batches, n_tiles // bt)
    import oracle_lib as O
    root = bytes(b"ACGT"[s & 3] for s in range(nchar))
    out = {"batches": [], "nchar": nchar, "batch_refs": BATCH}
    tmp = [dense_path + ".enc_a.uvdb", dense_path + ".enc_b.uvdb"]
    wa, wb = CL.create_compact(tmp[0], nchar), CL.create_compact(tmp[1], nchar)      # a: the parent's route (host encoder), b: the device route
    with capi.Engine.from_query(O.Query([root], ["q"]), nbest=1, max_pool=64, device=device) as eng:
        eng.db_reserve(BATCH)
        for b in range(n_batches):
            t0, t1 = b * bt, (b + 1) * bt
            planes = np.ascontiguousarray(mm[off_planes + t0 * tb:off_planes + t1 * tb]).reshape(bt, tb)
            non_n = np.ascontiguousarray(mm[off_nonn + t0 * 256:off_nonn + t1 * 256]).view(np.int32)
            side = np.ascontiguousarray(mm[off_side + t0 * 64 * 256:off_side + t1 * 64 * 256]).view(np.int32).reshape(bt * 64, 64)
            for w in (wa, wb):
                for i in range(BATCH):
                    L.uvdb_add_reference_runs(w, b"r%d" % (t0 * 64 + i), None, 0)
            eng.db_clear()
            eng.db_append_packed(planes, non_n, side, BATCH)
            eng.sync()
            c0 = time.perf_counter()
            p, nn, sd = eng.db_export(0, bt)
            c1 = time.perf_counter()
            assert L.uvdb_add_tiles(wa, bt, p.ctypes.data, nn.ctypes.data, None) == 0
            c2 = time.perf_counter()
            base_ptr = L.uvdb_compact_base(wb)
            if not base_ptr:                                             # the first batch fixes the base on either route
                assert L.uvdb_add_tiles(wb, bt, p.ctypes.data, nn.ctypes.data, None) == 0
                continue
            base = np.ctypeslib.as_array(C.cast(base_ptr, C.POINTER(C.c_uint32)), shape=(tb // 256,)).copy()
            eng.encode_ms(reset=True)
            c3 = time.perf_counter()
            hi, li, nn2 = eng.db_encode_compact(base, 0, bt)
            heads, lits = eng.db_encoded_records()
            c4 = time.perf_counter()
            hs = heads if heads.size else np.zeros(1, np.uint32)
            ls = lits if lits.size else np.zeros(4, np.uint32)
            assert L.uvdb_add_tiles_encoded(wb, bt, nn2.ctypes.data, hi.ctypes.data, hs.ctypes.data, li.ctypes.data, ls.ctypes.data) == 0
            c5 = time.perf_counter()
            ms = eng.encode_ms()
            copied = 4 * int(hi[-1]) + 16 * int(li[-1]) + 2 * 8 * (BATCH + 1) + 4 * BATCH
            out["batches"].append({"first_ref": t0 * 64, "device_count_prefix_ms": round(ms[0], 4), "device_emit_ms": round(ms[1], 4),
                                   "new_route_engine_calls_wall_ms": round(1e3 * (c4 - c3), 3), "new_route_writer_wall_ms": round(1e3 * (c5 - c4), 3),
                                   "parent_route_db_export_wall_ms": round(1e3 * (c1 - c0), 3), "parent_route_host_encoder_wall_ms": round(1e3 * (c2 - c1), 3),
                                   "heads": int(hi[-1]), "literal_words": int(li[-1]), "bytes_to_host_per_ref": round(copied / BATCH, 1)})
    assert L.uvdb_close(wa) == 0 and L.uvdb_close(wb) == 0
    out["files_equal"] = same(tmp[0], tmp[1])
    for t in tmp:
        os.remove(t)
    bs = out["batches"]
    if bs:
        med = lambda k: round(statistics.median(x[k] for x in bs), 4)
        out["median"] = {k: med(k) for k in bs[0] if k != "first_ref"}
        out["median"]["parent_route_wall_ms"] = round(out["median"]["parent_route_db_export_wall_ms"] + out["median"]["parent_route_host_encoder_wall_ms"], 3)
        out["median"]["new_route_wall_ms"] = round(out["median"]["new_route_engine_calls_wall_ms"] + out["median"]["new_route_writer_wall_ms"], 3)
        out["bytes_to_host_per_ref"] = {"compact_records_indices_counts": out["median"]["bytes_to_host_per_ref"], "dense_tile_side_row_count": DENSE_BYTES_PER_REF(nchar)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", required=True, help="directory with the parent commit's uvaiapack, uvaialign and uvaiaclust")
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--align-seqs", type=int, default=100000)
    ap.add_argument("--clust-refs", type=int, default=12000)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dir", default="/tmp/compact_encode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_encode.json"))
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    P = lambda name: os.path.join(a.dir, name)
    new = {k: os.path.join(ROOT, "bin", k) for k in ("uvaiapack", "uvaialign", "uvaiaclust")}
    old = {k: os.path.join(a.parent_bin, k) for k in new}
    doc = {"refs": a.refs, "align_seqs": a.align_seqs, "clust_refs": a.clust_refs, "repeats": a.repeats, "nchar": 29903,
           "not_measured": ["a cold page cache", "a run of 10 M rows"], "whole_commands": {}}

    # ---- the generator's genomes as text, and the dense file of them (the input of (b) and of the clustering)
    gen = hostlib.Synth()
    fa = P("refs.fa")
    with open(fa, "wb") as fh:
        for first in range(0, a.refs, 2048):
            rows, _ = gen.generate(first, min(2048, a.refs - first))
            for i in range(rows.shape[0]):
                fh.write(b">ref_%d\n" % (first + i) + rows[i].tobytes() + b"\n")
    run([new["uvaiapack"], "-o", P("dense.uvdb"), fa])

    # ---- (a) uvaiapack --compact
    last = {}

    def pack(which, exe):
        def f():
            w, err = run([exe, "--compact", "-o", P("pack_%s.uvdb" % which), fa])
            last[which] = routes(err)
            return w
        return f
    res = alternate({"parent": pack("parent", old["uvaiapack"]), "new": pack("new", new["uvaiapack"])}, a.repeats)
    doc["whole_commands"]["uvaiapack_compact"] = dict(res, files_equal=same(P("pack_parent.uvdb"), P("pack_new.uvdb")), new_tiles_by_route=last.get("new"),
                                                      file_bytes=os.path.getsize(P("pack_new.uvdb")), **verdict(res["parent"], res["new"]))

    # ---- (a) uvaialign --packed --compact against uvaialign --packed + uvaiapack --merge --compact
    if a.align_seqs > 0:
        g1 = hostlib.Synth(29903, seed=20241008, preset=1)
        ref = np.array(g1.generate(7, 1)[0][0], dtype=np.uint8)
        ref[~np.isin(ref, np.frombuffer(b"ACGT", dtype=np.uint8))] = ord("A")
        rng = np.random.default_rng(20241008)
        with open(P("ref.fa"), "wb") as fh:
            fh.write(b">reference\n" + ref.tobytes() + b"\n")
        n = 0
        with open(P("raw.fa"), "wb") as fh:
            for first in range(0, a.align_seqs, 2048):
                rows, _ = gen.generate(bench.QUERY_INDEX0 + first, min(2048, a.align_seqs - first))
                for s in bench.unaligned_from_rows(np.asarray(rows, dtype=np.uint8), rng):
                    fh.write(b">q_%d\n" % n + s + b"\n")
                    n += 1
        common = ["-r", P("ref.fa"), P("raw.fa"), "-a", "1.0", "-p", "4096"]

        def align_parent():
            w1, _ = run([old["uvaialign"]] + common + ["--packed", P("align_parent_dense.uvdb")])
            w2, _ = run([old["uvaiapack"], "--merge", "--compact", "-o", P("align_parent.uvdb"), P("align_parent_dense.uvdb")])
            return w1 + w2

        def align_new():
            w, err = run([new["uvaialign"]] + common + ["--packed", P("align_new.uvdb"), "--compact"])
            last["align"] = routes(err)
            return w
        res = alternate({"parent_two_commands": align_parent, "new": align_new}, a.repeats)
        doc["whole_commands"]["uvaialign_packed_compact"] = dict(res, sequences=n, files_equal=same(P("align_parent.uvdb"), P("align_new.uvdb")), new_tiles_by_route=last.get("align"),
                                                                 dense_bytes_the_parent_writes_and_reads_back=os.path.getsize(P("align_parent_dense.uvdb")),
                                                                 file_bytes=os.path.getsize(P("align_new.uvdb")), **verdict(res["parent_two_commands"], res["new"]))
    else:
        doc["not_measured"].append("uvaialign --packed --compact")

    # ---- (a) uvaiaclust --packed-out --compact against uvaiaclust --packed-out + uvaiapack --merge --compact
    if a.clust_refs > 0:
        with open(P("clust.fa"), "wb") as fh, open(fa, "rb") as src:
            for _ in range(2 * min(a.clust_refs, a.refs)):
                fh.write(src.readline())
        run([new["uvaiapack"], "-o", P("clust_in.uvdb"), P("clust.fa")])
        cargs = ["-d", "1", "-p", "64", "--packed", P("clust_in.uvdb")]

        def clust_parent():
            w1, _ = run([old["uvaiaclust"]] + cargs + ["--packed-out", P("clust_parent_dense.uvdb"), "-o", P("clust_parent")])
            w2, _ = run([old["uvaiapack"], "--merge", "--compact", "-o", P("clust_parent.uvdb"), P("clust_parent_dense.uvdb")])
            return w1 + w2

        def clust_new():
            w, err = run([new["uvaiaclust"]] + cargs + ["--packed-out", P("clust_new.uvdb"), "--compact", "-o", P("clust_new")])
            last["clust"] = routes(err)
            return w
        res = alternate({"parent_two_commands": clust_parent, "new": clust_new}, a.repeats)
        doc["whole_commands"]["uvaiaclust_packed_out_compact"] = dict(res, references=min(a.clust_refs, a.refs), files_equal=same(P("clust_parent.uvdb"), P("clust_new.uvdb")),
                                                                      new_tiles_by_route=last.get("clust"), file_bytes=os.path.getsize(P("clust_new.uvdb")),
                                                                      **verdict(res["parent_two_commands"], res["new"]))
    else:
        doc["not_measured"].append("uvaiaclust --packed-out --compact")

    # ---- (b), (c)
    doc["per_batch"] = per_batch(P("dense.uvdb"), a.batches, a.device)
    os.remove(fa)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    bad = [k for k, v in doc["whole_commands"].items() if not v["files_equal"]] + ([] if doc["per_batch"]["files_equal"] else ["per_batch"])
    if bad:
        sys.exit("different files: %s" % bad)


if __name__ == "__main__":
    main()
