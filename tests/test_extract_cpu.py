"""Rows out of a packed database, the part that needs no GPU: what `uvaia --final-aln` and `uvaiapack --unpack / --names / --list` refuse
while they read their options (before a GPU is touched or a file written), `uvaiapack --list`, and the chunk planner and the name
table of uvaia_amd/csrc/host/uvdb_extract.c through the host library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compact_lib as CL
import packed_lib as P
from uvaia_amd import capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIA = os.path.join(ROOT, "bin", "uvaia")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")
NCHAR = 130


def _refused(cmd, word, absent):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0, cmd
    assert word in r.stderr, (cmd, r.stderr[-2000:])
    assert b"HIP device" not in r.stderr, (cmd, r.stderr[-2000:])     # refused on its own grounds, not for the missing GPU
    for p in absent:
        assert not os.path.exists(p), (cmd, p)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """a dense file of 70 references, a compact one of 130 (names a*, b*), a query and a text reference file"""
    hostlib.build_library()
    d = tmp_path_factory.mktemp("extract_cpu")
    out = {}
    for tag, n, compact in (("a", 70, False), ("b", 130, True)):
        seqs = [s.upper() for s in P.awkward_references(n, NCHAR, 40 + n)]
        names = ["%s%d" % (tag, i) for i in range(n)]
        planes, non_n = P.pack_tiles(seqs, NCHAR)
        path = d / ("%s.uvdb" % tag)
        if compact:
            CL.write_compact(path, names, seqs, planes, non_n)
        else:
            P.write_uvdb(path, names, seqs, planes, non_n, CL.side_rows_canonical(planes, NCHAR))
        out[tag] = (str(path), names)
    (d / "q.fa").write_bytes(b">q0\n" + b"ACGT" * 32 + b"AC\n")
    (d / "r.fa").write_bytes(b">r0\n" + b"ACGT" * 32 + b"AC\n>r1\n" + b"ACGA" * 32 + b"AC\n")
    (d / "names.txt").write_bytes(b"a3\n")
    return d, out


def test_uvaia_refuses_final_options_while_it_reads_them(files):
    d, f = files
    q, db = str(d / "q.fa"), f["a"][0]
    made = lambda p: [p + s for s in (".aln.xz", ".csv.xz", ".final.aln.xz")]
    p = str(d / "u1")
    _refused([UVAIA, q, "-r", str(d / "r.fa"), "--final-aln", "-o", p], b"uvaiapack", made(p))
    _refused([UVAIA, q, "-r", str(d / "r.fa"), "--final-aln", "-o", p], b"--final-aln needs --packed", made(p))
    p = str(d / "u2")
    _refused([UVAIA, q, "--packed", db, "--final-rank", "2", "-o", p], b"--final-rank needs --final-aln", made(p))
    p = str(d / "u3")
    _refused([UVAIA, q, "--packed", db, "--final-only", "-o", p], b"--final-only needs --final-aln", made(p))
    p = str(d / "u4")
    for bad in ("0", "-3"):
        _refused([UVAIA, q, "--packed", db, "--final-aln", "--final-rank", bad, "-o", p], b"--final-rank: expected a rank of 1 or more", made(p))
    p = str(d / "u5")
    _refused([UVAIA, q, "--packed", db, "--final-aln", "--devices", "0,1", "-o", p], b"--final-aln works on one GPU", made(p))
    _refused([UVAIA, q, "--packed", db, "--final-aln", "--final-only", "--devices", "0-3", "-o", p], b"--final-aln works on one GPU", made(p))


def test_uvaiapack_refuses_option_conflicts_while_it_reads_them(files):
    d, f = files
    a, b, names = f["a"][0], f["b"][0], str(d / "names.txt")
    p = str(d / "p1")
    made = [p, p + ".aln.xz"]
    word = b"--unpack writes the references as they are stored"
    _refused([UVAIAPACK, "--unpack", "--merge", "-o", p, a], word, made)
    _refused([UVAIAPACK, "--unpack", "--compact", "-o", p, a], word, made)
    _refused([UVAIAPACK, "--unpack", "-A", "0.5", "-o", p, a], word, made)
    _refused([UVAIAPACK, "--unpack", "--stdout", "--merge", a], word, made)
    word = b"--unpack needs exactly one of -o <prefix> and --stdout"
    _refused([UVAIAPACK, "--unpack", a], word, made)
    _refused([UVAIAPACK, "--unpack", "-o", p, "--stdout", a, b], word, made)
    _refused([UVAIAPACK, "--names", names, "-o", p, a], b"--names needs --unpack", made)
    _refused([UVAIAPACK, "--merge", "--names", names, "-o", p, a], b"--names needs --unpack", made)
    word = b"--list prints the stored names and takes no other option"
    for other in (["--unpack", "--stdout"], ["--merge", "-o", p], ["--compact", "-o", p], ["-A", "0.5"], ["-o", p], ["--stdout"], ["--names", names]):
        _refused([UVAIAPACK, "--list"] + other + [a], word, made)


def test_list_prints_the_stored_names_in_stream_order(files):
    d, f = files
    (a, an), (b, bn) = f["a"], f["b"]
    assert CL.file_version(a) == 1 and CL.file_version(b) == 2
    for paths, want in (([a], an), ([b], bn), ([b, a], bn + an)):
        r = subprocess.run([UVAIAPACK, "--list"] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.decode().split("\n") == want + [""]
        assert b"HIP" not in r.stderr


# ------------------------------------------------------------------------------------------------------ the planner and the name table
class _Piece(C.Structure):
    _fields_ = [("file", C.c_int), ("first_tile", C.c_uint64), ("n_tiles", C.c_uint64), ("slot_tile", C.c_uint64)]


def _host():
    L = hostlib.load_library()
    L.uvdb_set_open.restype = C.c_void_p
    L.uvdb_set_open.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.uvdb_set_close.argtypes = [C.c_void_p]
    L.uvdb_set_close.restype = None
    L.uvdb_extract_plan.restype = C.c_int
    L.uvdb_extract_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(_Piece), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    return L


def _plan(L, s, pos, a, b, max_pieces=256):
    arr = None if pos is None else np.ascontiguousarray(pos, dtype=np.uint64)
    pieces, np_, st, sel = (_Piece * max_pieces)(), C.c_int(0), C.c_uint64(0), (C.c_int * max(b - a, 1))()
    rc = L.uvdb_extract_plan(s, None if arr is None else arr.ctypes.data, a, b, pieces, max_pieces, C.byref(np_), C.byref(st), sel)
    if rc:
        return None
    return [(p.file, p.first_tile, p.n_tiles, p.slot_tile) for p in pieces[:np_.value]], st.value, list(sel[:b - a])


def test_the_chunk_plan_stages_only_the_tiles_it_needs(files):
    d, f = files
    L = _host()
    paths = (C.c_char_p * 2)(f["a"][0].encode(), f["b"][0].encode())              # 70 references (two tiles), then 130 (three tiles)
    err = C.create_string_buffer(512)
    s = L.uvdb_set_open(paths, 2, 0, err, 512)
    assert s, err.value
    try:
        # the whole stream: a's two tiles, b's three, one piece per file; a's second tile holds 6 references
        pieces, st, sel = _plan(L, s, None, 0, 200)
        assert pieces == [(0, 0, 2, 0), (1, 0, 3, 2)] and st == 5
        assert sel == list(range(70)) + [128 + i for i in range(130)]
        # far apart: tiles in between are not staged, a tile shared by two positions is staged once
        pos = [0, 3, 69, 70, 70 + 128, 70 + 129]
        pieces, st, sel = _plan(L, s, pos, 0, len(pos))
        assert pieces == [(0, 0, 2, 0), (1, 0, 1, 2), (1, 2, 1, 3)] and st == 4
        assert sel == [0, 3, 64 + 5, 128, 192, 193]
        # a range in the middle of the list
        pieces, st, sel = _plan(L, s, pos, 2, 5)
        assert pieces == [(0, 1, 1, 0), (1, 0, 1, 1), (1, 2, 1, 2)] and sel == [5, 64, 128]
        # refused: a repeat, a descent, a position outside the stream, an empty range, more positions than pieces
        assert _plan(L, s, [5, 5], 0, 2) is None
        assert _plan(L, s, [6, 5], 0, 2) is None
        assert _plan(L, s, [199, 200], 0, 2) is None
        assert _plan(L, s, None, 190, 201) is None
        assert _plan(L, s, [1], 0, 0) is None
        assert _plan(L, s, None, 0, 5, max_pieces=4) is None
    finally:
        L.uvdb_set_close(s)


def test_the_name_table(tmp_path):
    L = hostlib.load_library()
    L.uvdb_name_list_read.restype = C.c_void_p
    L.uvdb_name_list_read.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.uvdb_name_list_find.restype = C.c_long
    L.uvdb_name_list_find.argtypes = [C.c_void_p, C.c_char_p]
    L.uvdb_name_list_free.argtypes = [C.c_void_p]
    L.uvdb_name_list_free.restype = None
    err = C.create_string_buffer(512)
    assert not L.uvdb_name_list_read(str(tmp_path / "absent.txt").encode(), err, 512) and b"absent.txt" in err.value
    p = tmp_path / "n.txt"
    p.write_bytes(b"zeta\r\n\nalpha\nhCoV-19/x y|2020\nalpha\nlast-without-newline")
    l = L.uvdb_name_list_read(str(p).encode(), err, 512)
    assert l, err.value
    try:
        found = {n: L.uvdb_name_list_find(l, n) for n in (b"alpha", b"zeta", b"hCoV-19/x y|2020", b"last-without-newline")}
        assert sorted(found.values()) == [0, 1, 2, 3]                               # four distinct names: the repeat and the empty line are gone
        for n in (b"", b"alph", b"alphaa", b"zeta\r", b"hCoV-19/x"):
            assert L.uvdb_name_list_find(l, n) == -1
    finally:
        L.uvdb_name_list_free(l)


def test_the_new_entry_is_exported_and_the_header_stays_plain_c(tmp_path):
    lib = capi.load_library()
    for name in ("uvaia_gpu_db_stage_unpack_rows", "uvaia_gpu_stage_unpack_ms"):
        assert name in capi.SYMBOLS
        assert hasattr(lib, name), name
    assert callable(capi.Engine.db_stage_unpack_rows) and callable(capi.Engine.stage_unpack_ms)
    src = tmp_path / "t.c"
    src.write_text('#include "uvaia_gpu.h"\n'
                   "int (*rows) (uvaia_gpu_ctx *, int, const int *, int, char *, size_t) = uvaia_gpu_db_stage_unpack_rows;\n"
                   "double (*ms) (uvaia_gpu_ctx *, int) = uvaia_gpu_stage_unpack_ms;\n"
                   "int main (void) { return rows == 0 || ms == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
    assert lib.uvaia_gpu_db_stage_unpack_rows(None, 0, None, 0, None, 0) == -1      # no context: an error, not a fault
