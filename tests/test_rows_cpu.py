"""`uvaialign --packed` without a GPU: the writer entry that takes exception runs instead of text, the declarations and exports of the new C
entries, and the refusals of the command line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import packed_lib as P
import rows_lib as R
from uvaia_amd import align, capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIALIGN = os.path.join(ROOT, "bin", "uvaialign")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")

NEW_GPU = ["uvaia_gpu_rows_census", "uvaia_gpu_db_append_device", "uvaia_gpu_rows_exceptions", "uvaia_gpu_db_drop_tiles"]
NEW_ALIGN = ["uvaia_align_device_rows"]


# ------------------------------------------------------------------------------------------------------------ writer equivalence
def _case_rows(nchar=200):
    rng = np.random.default_rng(5)
    base = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nchar))

    def put(s, at, what):
        return s[:at] + what + s[at + len(what):]

    rows = [
        put(put(base, 0, b"-----"), nchar - 7, b"???????"),                    # runs at site 0 and at the last site
        put(base, 50, b"---...XXXOOO??-"),                                     # adjacent runs of different characters
        put(base, 30, b"----N----"),                                           # N between two '-' runs
        put(base, 70, b"xxxooo-xo-"),                                          # lower-case x and o are no exceptions
        base,                                                                  # no run
        b"-" * nchar,                                                          # one single run
        b"." + base[1:nchar - 1] + b"X",                                       # runs of one site at both ends
    ]
    return rows + R.random_rows(40, nchar, seed=9)


def _write(path, rows, nchar, by_runs):
    L = P._lib()
    L.uvdb_add_reference_runs.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
    L.uvdb_add_reference_runs.restype = C.c_int
    planes, non_n = P.pack_tiles([bytes(ord("N") if c in P.EXCEPTIONS else c for c in r) for r in rows], nchar)
    side = np.zeros((planes.shape[0] * 64, P.SIDE_ROW_INTS), dtype=np.int32)
    w = L.uvdb_create(str(path).encode(), nchar, P.tile_bytes(nchar), P.SIDE_ROW_INTS, 0.5)
    assert w
    for i, r in enumerate(rows):
        name = ("ref/%d" % i).encode()
        if by_runs:
            runs = np.array(R.exception_runs(r), dtype=np.uint32).reshape(-1, 2)
            assert L.uvdb_add_reference_runs(w, name, runs.ctypes.data if len(runs) else None, len(runs)) == 0
        else:
            assert L.uvdb_add_reference(w, name, r) == 0
    assert L.uvdb_add_tiles(w, planes.shape[0], planes.ctypes.data, non_n.ctypes.data, side.ctypes.data) == 0
    assert L.uvdb_close(w) == 0


def test_the_restated_run_rule_on_the_named_cases():
    rows = _case_rows()
    ch = lambda n, c: (n << 8) | ord(c)
    assert R.exception_runs(rows[0]) == [(0, ch(5, "-")), (193, ch(7, "?"))]
    assert R.exception_runs(rows[1]) == [(50, ch(3, "-")), (53, ch(3, ".")), (56, ch(3, "X")), (59, ch(3, "O")), (62, ch(2, "?")), (64, ch(1, "-"))]
    assert R.exception_runs(rows[2]) == [(30, ch(4, "-")), (35, ch(4, "-"))]
    assert R.exception_runs(rows[3]) == [(76, ch(1, "-")), (79, ch(1, "-"))]
    assert R.exception_runs(rows[4]) == []
    assert R.exception_runs(rows[5]) == [(0, ch(200, "-"))]
    assert R.exception_runs(b"A" + b"-" * 11 + b"C", cut=5) == [(1, ch(5, "-")), (6, ch(5, "-")), (11, ch(1, "-"))]
    assert [R.count_non_n(r) for r in (b"ACGTNnXxOo-?.", b"acgtMRWSYKVHDB", b"")] == [4, 14, 0]


def test_writer_fed_runs_writes_the_file_the_writer_fed_text_writes(tmp_path):
    hostlib.build_library()
    rows = _case_rows()
    nchar = len(rows[0])
    _write(tmp_path / "text.uvdb", rows, nchar, by_runs=False)
    _write(tmp_path / "runs.uvdb", rows, nchar, by_runs=True)
    a, b = (tmp_path / "text.uvdb").read_bytes(), (tmp_path / "runs.uvdb").read_bytes()
    assert a == b
    rd = P.Reader(tmp_path / "runs.uvdb", nchar)                              # ... and the text comes back out of it
    for i, r in enumerate(rows):
        assert rd.apply_exceptions(i, bytes(ord("N") if c in P.EXCEPTIONS else c for c in r)) == r
    rd.close()


# ------------------------------------------------------------------------------------------------------------ headers and exports
def test_new_entries_are_declared_bound_and_exported():
    capi.build_library()
    lib = capi.load_library()
    gpu_h = open(os.path.join(ROOT, "include", "uvaia_gpu.h")).read()
    align_h = open(os.path.join(ROOT, "include", "uvaia_align.h")).read()
    for name in NEW_GPU:
        assert re.search(r"\bint\s+%s\s*\(" % name, gpu_h), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for name in NEW_ALIGN:
        assert re.search(r"\bint\s+%s\s*\(" % name, align_h), name
        assert name in align.SYMBOLS and hasattr(lib, name), name
    host_h = open(os.path.join(ROOT, "uvaia_amd", "csrc", "host", "uvdb.h")).read()
    assert re.search(r"\bint\s+uvdb_add_reference_runs\s*\(", host_h)
    assert hasattr(hostlib.load_library(), "uvdb_add_reference_runs")


def test_library_holds_the_three_kernels_for_gfx950():
    """the hot path is device code of its own: the kernels are in the library's gfx950 code object"""
    capi.build_library()
    blob = open(capi.library_path(), "rb").read()
    for kernel in (b"rows_census_kernel", b"rows_fill_exceptions_kernel", b"rows_gather_kernel"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob


def test_headers_with_the_new_entries_are_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "uvaia_gpu.h"\n#include "uvaia_align.h"\n#include "uvdb.h"\n'
                   "int main(void){ int (*a)(uvaia_gpu_ctx *, const void *, size_t, int, int *, int *) = uvaia_gpu_rows_census;\n"
                   "  int (*b)(uvaia_gpu_ctx *, const void *, size_t, const int *, int, const int *) = uvaia_gpu_db_append_device;\n"
                   "  int (*c)(uvaia_gpu_ctx *, const void *, size_t, const int *, int, const uint64_t *, void *) = uvaia_gpu_rows_exceptions;\n"
                   "  int (*d)(uvaia_aligner *, const void **, size_t *, int *, int *) = uvaia_align_device_rows;\n"
                   "  int (*e)(uvdb_writer, const char *, const uvdb_exc *, size_t) = uvdb_add_reference_runs;\n"
                   "  return !(a && b && c && d && e); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "uvaia_amd", "csrc", "host"), "-c", str(src), "-o", str(tmp_path / "t.o")])


# ------------------------------------------------------------------------------------------------------------ command line
@pytest.fixture(scope="module")
def tools():
    capi.build_library()
    hostlib.build_library()
    assert os.path.exists(UVAIALIGN)


def _cli(args):
    r = subprocess.run([UVAIALIGN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return r.returncode, r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")


def test_packed_without_a_value_is_a_usage_error(tools):
    rc, out, err = _cli(["-r", "ref.fa", "seqs.fa", "--packed"])
    assert rc != 0
    assert "The complete syntax is" in out and "--packed" in out


def test_packed_with_several_devices_is_refused_before_a_device_is_opened(tools, tmp_path):
    ref = tmp_path / "ref.fa"                                    # (the files do not exist: the refusal comes before anything is read)
    rc, out, err = _cli(["--packed", str(tmp_path / "x.uvdb"), "--devices", "0,1", "-r", str(ref), str(tmp_path / "seqs.fa")])
    assert rc != 0
    assert "--packed" in err and "ONE GPU" in err
    assert "HIP" not in err and "device 0" not in err and "program:" not in err
    assert not (tmp_path / "x.uvdb").exists()


def test_help_lists_the_new_options(tools):
    rc, out, err = _cli(["-h"])
    assert rc == 0
    assert "--packed=<out.uvdb>" in out and "-A, --ref_ambiguity=<double>" in out
    pack_help = subprocess.run([UVAIAPACK, "-h"], stdout=subprocess.PIPE, timeout=120).stdout.decode()
    assert "uvaialign --packed" in pack_help
