"""Host-side pieces of the device-encoded compact packed database that need no GPU: the writer's entry for records somebody else encoded
(uvdb_compact_base, uvdb_add_tiles_encoded in uvaia_amd/csrc/host/uvdb.h), the new entries of the C ABI, and the refusals `uvaialign
--compact` and `uvaiaclust --compact` make before they open a GPU.  The reference of every comparison is the file the host writer
(compact_lib.write_compact) makes of the same rows; the records handed to the new entry are sliced out of that file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compact_lib as CL
import packed_lib as PL
from uvaia_amd import capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCHAR = 200


def _lib():
    hostlib.build_library()
    L = CL._lib()
    L.uvdb_compact_base.restype = C.c_void_p
    L.uvdb_compact_base.argtypes = [C.c_void_p]
    L.uvdb_add_tiles_encoded.restype = C.c_int
    L.uvdb_add_tiles_encoded.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def host_files(tmp_path_factory):
    """{n: (path of the host-written file, names, seqs, planes, non_n)} -- written once, never changed"""
    _lib()
    d = tmp_path_factory.mktemp("compact_encode_cpu")
    out = {}
    for n in (4097, 4300):
        seqs = CL.near_identical_references(n, NCHAR, seed=n)
        names = ["r%d" % i for i in range(n)]
        planes, non_n = PL.pack_tiles(seqs, NCHAR)
        path = d / ("host_%d.uvdb" % n)
        CL.write_compact(path, names, seqs, planes, non_n)
        out[n] = (path, names, seqs, planes, non_n)
    return out


def _dense_until_base(L, w, names, seqs, planes, non_n):
    """tile by tile through uvdb_add_tiles until the base is fixed; the number of tiles that took"""
    n_tiles = planes.shape[0]
    for t in range(n_tiles):
        assert not L.uvdb_compact_base(w)
        for nm, s in zip(names[t * 64:(t + 1) * 64], seqs[t * 64:(t + 1) * 64]):
            assert L.uvdb_add_reference(w, nm.encode(), s) == 0
        p, nn = np.ascontiguousarray(planes[t:t + 1]), np.ascontiguousarray(non_n[t * 64:(t + 1) * 64])
        assert L.uvdb_add_tiles(w, 1, p.ctypes.data, nn.ctypes.data, None) == 0
        if L.uvdb_compact_base(w):
            return t + 1
    raise AssertionError("the base was never fixed")


def _add_encoded(L, w, f, t0, nt, heads=None, head_idx=None, lit_idx=None, rebase=False):
    """tiles t0 .. t0 + nt - 1 of CompactFile f as records; rebase: offsets from 0 and arrays that start at the chunk, as the engine gives them"""
    hi = np.ascontiguousarray((f.head_idx if head_idx is None else head_idx)[t0 * 64:(t0 + nt) * 64 + 1])
    li = np.ascontiguousarray((f.lit_idx if lit_idx is None else lit_idx)[t0 * 64:(t0 + nt) * 64 + 1])
    hs = f.heads if heads is None else heads
    ls = f.lits
    if rebase:
        hs = np.ascontiguousarray(hs[int(hi[0]):int(hi[-1])])
        ls = np.ascontiguousarray(ls[int(li[0]) * 4:int(li[-1]) * 4])
        hi, li = hi - hi[0], li - li[0]
    hs = hs if hs.size else np.zeros(1, dtype=np.uint32)
    ls = ls if ls.size else np.zeros(4, dtype=np.uint32)
    nn = np.ascontiguousarray(f.non_n[t0 * 64:(t0 + nt) * 64])
    return L.uvdb_add_tiles_encoded(w, nt, nn.ctypes.data, hi.ctypes.data, hs.ctypes.data, li.ctypes.data, ls.ctypes.data)


@pytest.mark.parametrize("n", [4097, 4300])
@pytest.mark.parametrize("chunk,rebase", [(1, False), (3, True), (None, False), (None, True)])
def test_a_spliced_file_equals_the_host_written_one(host_files, tmp_path, n, chunk, rebase):
    L = _lib()
    path, names, seqs, planes, non_n = host_files[n]
    f = CL.CompactFile(path)
    assert f.n_ref == n and n % 64 != 0                      # both counts end inside a tile: zero lanes behind the last reference
    out = tmp_path / "spliced.uvdb"
    w = CL.create_compact(out, NCHAR)
    assert w
    t = _dense_until_base(L, w, names, seqs, planes, non_n)
    assert t == CL.BASE_SAMPLE // 64 and t < f.n_tiles
    base = np.ctypeslib.as_array(C.cast(L.uvdb_compact_base(w), C.POINTER(C.c_uint32)), shape=(f.W4 * 16,))
    assert np.array_equal(base, f.base)
    for nm, s in zip(names[t * 64:], seqs[t * 64:]):
        assert L.uvdb_add_reference(w, nm.encode(), s) == 0
    step = f.n_tiles - t if chunk is None else chunk
    while t < f.n_tiles:
        nt = min(step, f.n_tiles - t)
        assert _add_encoded(L, w, f, t, nt, rebase=rebase) == 0
        t += nt
    assert L.uvdb_close(w) == 0
    assert out.read_bytes() == path.read_bytes()


def test_encoded_tiles_are_refused_before_the_base_is_fixed_and_by_a_dense_writer(host_files, tmp_path):
    L = _lib()
    path, names, seqs, planes, non_n = host_files[4097]
    f = CL.CompactFile(path)
    w = CL.create_compact(tmp_path / "early.uvdb", NCHAR)
    assert not L.uvdb_compact_base(w)
    assert _add_encoded(L, w, f, 0, 1) == -1
    for nm, s in zip(names[:64], seqs[:64]):
        assert L.uvdb_add_reference(w, nm.encode(), s) == 0
    p, nn = np.ascontiguousarray(planes[:1]), np.ascontiguousarray(non_n[:64])
    assert L.uvdb_add_tiles(w, 1, p.ctypes.data, nn.ctypes.data, None) == 0
    assert not L.uvdb_compact_base(w) and _add_encoded(L, w, f, 1, 1) == -1        # 64 references: the sample is not complete
    assert L.uvdb_close(w) == 0
    dense = PL._lib().uvdb_create(str(tmp_path / "dense.uvdb").encode(), NCHAR, PL.tile_bytes(NCHAR), PL.SIDE_ROW_INTS, 0.5)
    assert dense and not L.uvdb_compact_base(dense) and _add_encoded(L, dense, f, 0, 1) == -1
    assert L.uvdb_close(dense) == 0


def _damaged(f, t0):
    """{what: (heads, head_idx, lit_idx)} -- the records of the file with one lane behind tile t0 damaged in one way"""
    lanes = range(t0 * 64, f.lanes)
    two = next(g for g in lanes if len(f.heads_of(g)) >= 2 and not f.heads_of(g)[0][2] and f.heads_of(g)[1][0] > f.heads_of(g)[0][0] + f.heads_of(g)[0][1])
    lit = next(g for g in lanes if any(h[2] for h in f.heads_of(g)))
    any_ = next(g for g in lanes if f.heads_of(g))
    out = {}
    h = f.heads.copy(); k = int(f.head_idx[two]); h[k], h[k + 1] = h[k + 1], h[k]
    out["descending"] = (h, None, None)
    h = f.heads.copy(); a, b = f.heads_of(two)[0], f.heads_of(two)[1]
    h[k] = CL.head(a[0], b[0] - a[0] + 1, a[2], a[3])                             # a fill that reaches into the next head's first word
    out["overlap"] = (h, None, None)
    h = f.heads.copy(); k = int(f.head_idx[any_]); h[k] &= ~np.uint32(0x7FF << 5)
    out["empty"] = (h, None, None)
    h = f.heads.copy(); k = int(f.head_idx[any_ + 1]) - 1; h[k] = CL.head(CL.n_words(f.nchar) - 1, 2, 0, 0)
    out["leaves the alignment"] = (h, None, None)
    h = f.heads.copy(); k = int(f.head_idx[lit]) + next(i for i, x in enumerate(f.heads_of(lit)) if x[2]); h[k] &= ~np.uint32(1 << 4)
    out["literal count"] = (h, None, None)
    li = f.lit_idx.copy(); li[lit + 1:] += 1                                       # the lane's extent of lits one word longer than its heads say
    out["literal extent"] = (None, None, li)
    hi = f.head_idx.copy(); hi[any_ + 1] = hi[any_] - 1 if hi[any_] else hi[-1] + 1
    out["index"] = (None, hi, None)
    return out


def test_damaged_records_are_refused_with_nothing_appended(host_files, tmp_path):
    L = _lib()
    path, names, seqs, planes, non_n = host_files[4300]
    f = CL.CompactFile(path)
    out = tmp_path / "after_refusals.uvdb"
    w = CL.create_compact(out, NCHAR)
    t = _dense_until_base(L, w, names, seqs, planes, non_n)
    for nm, s in zip(names[t * 64:], seqs[t * 64:]):
        assert L.uvdb_add_reference(w, nm.encode(), s) == 0
    rest = f.n_tiles - t
    cases = _damaged(f, t)
    assert len(cases) == 7
    for what, (heads, head_idx, lit_idx) in cases.items():
        assert _add_encoded(L, w, f, t, rest, heads=heads, head_idx=head_idx, lit_idx=lit_idx) == -1, what
    assert _add_encoded(L, w, f, t, rest) == 0                                     # the writer is as it was: the good records complete the file
    assert L.uvdb_close(w) == 0
    assert out.read_bytes() == path.read_bytes()
    assert CL.try_open(out)[0]


def test_the_new_entries_are_exported_and_the_header_stays_plain_c(tmp_path):
    lib = capi.load_library()
    for name in ("uvaia_gpu_db_encode_compact", "uvaia_gpu_db_encoded_records", "uvaia_gpu_encode_ms"):
        assert name in capi.SYMBOLS
        assert hasattr(lib, name), name
    for name in ("db_encode_compact", "db_encoded_records", "encode_ms"):
        assert callable(getattr(capi.Engine, name))
    host = _lib()
    for name in ("uvdb_compact_base", "uvdb_add_tiles_encoded", "uvdb_export_tiles", "uvdb_export_free"):
        assert hasattr(host, name), name
    src = tmp_path / "t.c"
    src.write_text('#include "uvaia_gpu.h"\n'
                   "int (*plan) (uvaia_gpu_ctx *, size_t, size_t, const void *, uint64_t *, uint64_t *, int *) = uvaia_gpu_db_encode_compact;\n"
                   "int (*records) (uvaia_gpu_ctx *, uint32_t *, void *) = uvaia_gpu_db_encoded_records;\n"
                   "void (*ms) (uvaia_gpu_ctx *, double *, int) = uvaia_gpu_encode_ms;\n"
                   "int main (void) { return plan == 0 || records == 0 || ms == 0 || UVAIA_GPU_COMPACT_MAX_NCHAR != 2097152; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
    lib.uvaia_gpu_db_encode_compact.restype = C.c_int
    lib.uvaia_gpu_db_encoded_records.restype = C.c_int
    assert lib.uvaia_gpu_db_encode_compact(None, 0, 0, None, None, None, None) == -1 and lib.uvaia_gpu_db_encoded_records(None, None, None) == -1    # no context: an error, not a fault


def _refused(cmd, word, absent):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0, cmd
    assert word in r.stderr, (cmd, r.stderr[-2000:])
    assert b"HIP device" not in r.stderr, (cmd, r.stderr[-2000:])     # refused on its own grounds, not for the missing GPU
    for p in absent:
        assert not os.path.exists(p), (cmd, p)


def test_the_commands_refuse_compact_misuse_before_they_need_a_gpu(tmp_path):
    hostlib.build_library()
    align, clust = os.path.join(ROOT, "bin", "uvaialign"), os.path.join(ROOT, "bin", "uvaiaclust")
    ref = tmp_path / "ref.fa"
    ref.write_bytes(b">ref\n" + b"ACGT" * 50 + b"\n")
    seqs = tmp_path / "s.fa"
    seqs.write_bytes(b">s0\n" + b"ACGT" * 50 + b"\n>s1\n" + b"ACGT" * 49 + b"ACGA\n")
    db = str(tmp_path / "out.uvdb")
    _refused([align, "--compact", "-r", str(ref), "-o", str(tmp_path / "a"), str(seqs)], b"--packed", [str(tmp_path / "a.aln.xz")])
    _refused([clust, "--compact", "-o", str(tmp_path / "c"), str(seqs)], b"--packed-out", [str(tmp_path / "c.aln.xz")])
    big = tmp_path / "big.fa"
    big.write_bytes(b">big\n" + b"ACGT" * (CL.MAX_NCHAR // 4) + b"A\n")                  # one site above the limit
    _refused([align, "--packed", db, "--compact", "-r", str(big), str(seqs)], b"--compact: alignments of more than 2097152 sites have no compact form (2097153 sites)", [db])
    _refused([clust, "--packed-out", db, "--compact", "-r", str(big), "-o", str(tmp_path / "c"), str(big)],
             b"--compact: alignments of more than 2097152 sites have no compact form (2097153 sites)", [db, str(tmp_path / "c.aln.xz")])
