"""Host-side pieces of `uvaia --packed --window` that need no GPU: the window plan (uvaia_amd/csrc/host/uvdb_window.h), the new entries of
the C ABI and the refusals the command makes before it opens a GPU."""
import ctypes as C
import os
import subprocess

import pytest

import fixtures as F
import packed_lib as P
from uvaia_amd import capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = C.c_uint64


@pytest.fixture(scope="module")
def L():
    hostlib.build_library()
    lib = hostlib.load_library()
    lib.uvdb_window_plan.restype = C.c_int
    lib.uvdb_window_plan.argtypes = [U64, U64, U64, C.POINTER(U64), C.POINTER(U64)]
    lib.uvdb_window_span.restype = C.c_int
    lib.uvdb_window_span.argtypes = [C.POINTER(U64), U64, U64, C.POINTER(U64), C.POINTER(U64), C.POINTER(C.c_int)]
    lib.uvdb_window_choose.restype = C.c_int64
    lib.uvdb_window_choose.argtypes = [U64, U64, U64, U64]
    return lib


def _plan(L, n_kept, pool, request):
    w, nw = U64(0), U64(0)
    rc = L.uvdb_window_plan(n_kept, pool, request, C.byref(w), C.byref(nw))
    return rc, w.value, nw.value


@pytest.mark.parametrize("pool,asked,window", [(64, 100, 128), (96, 100, 192), (128, 128, 128), (100, 1, 1600)])
def test_window_is_a_multiple_of_the_pool_and_of_a_tile(L, pool, asked, window):
    assert _plan(L, 10 ** 6, pool, asked)[:2] == (0, window)
    assert window % pool == 0 and window % 64 == 0 and window >= asked and window - asked < pool * 64


@pytest.mark.parametrize("n_kept,n_windows", [(0, 0), (1, 1), (192, 1), (193, 2), (384, 2), (385, 3)])
def test_windows_cover_the_kept_stream(L, n_kept, n_windows):
    assert _plan(L, n_kept, 96, 100) == (0, 192, n_windows)              # 192 = exactly one window


def test_plan_refuses_what_it_cannot_count(L):
    assert _plan(L, 10, 0, 100)[0] != 0 and _plan(L, 10, 64, 0)[0] != 0
    assert _plan(L, 10, 64, 1 << 31)[0] != 0                              # the engine counts a window in an int


def _span(L, keep, a, b):
    arr = None if keep is None else (U64 * len(keep))(*keep)
    t0, nt = U64(0), U64(0)
    sel = (C.c_int * (b - a))()
    assert L.uvdb_window_span(arr, a, b, C.byref(t0), C.byref(nt), sel) == 0
    t0b, ntb = U64(0), U64(0)
    assert L.uvdb_window_span(arr, a, b, C.byref(t0b), C.byref(ntb), None) == 0 and (t0b.value, ntb.value) == (t0.value, nt.value)
    return t0.value, nt.value, list(sel)


def _check_span(L, keep, a, b):
    t0, nt, sel = _span(L, keep, a, b)
    want = list(range(a, b)) if keep is None else keep[a:b]
    assert all(x < y for x, y in zip(sel, sel[1:]))                      # strictly increasing
    assert sel[0] >= 0 and sel[-1] < 64 * nt                             # inside the span
    assert [t0 * 64 + s for s in sel] == want                            # and back to keep[a .. b)
    assert t0 == want[0] // 64 and t0 + nt - 1 == want[-1] // 64         # no tile more than needed
    return t0, nt, sel


def test_span_cases(L):
    assert _check_span(L, None, 0, 256)[:2] == (0, 4)                     # keep NULL: the identity
    assert _check_span(L, None, 256, 444) == (4, 3, list(range(188)))     # ... and a window that ends inside a tile
    n_file = 700
    hole_lane0 = [i for i in range(n_file) if i != 64]                    # a hole at the first lane of a tile
    t0, nt, sel = _check_span(L, hole_lane0, 0, 256)
    assert (t0, nt) == (0, 5) and sel[64] == 65                           # 256 kept references reach into a fifth tile
    assert _check_span(L, hole_lane0, 256, 512)[:2] == (4, 5)             # the following window starts inside that tile
    whole_tile = [i for i in range(n_file) if not 128 <= i < 192]         # a whole file tile excluded
    t0, nt, sel = _check_span(L, whole_tile, 0, 256)
    assert (t0, nt) == (0, 5) and sel[127] == 127 and sel[128] == 192
    t0, nt, sel = _check_span(L, whole_tile, 128, 192)                    # a window that starts right behind the excluded tile
    assert (t0, nt) == (3, 1) and sel == list(range(64))
    last_hole = [i for i in range(n_file) if i != n_file - 1]             # a hole at the last kept reference
    t0, nt, sel = _check_span(L, last_hole, 512, len(last_hole))
    assert (t0, nt) == (8, 3) and sel[-1] == (n_file - 2) - 512
    assert _check_span(L, [5, 700, 7000], 0, 3)[:2] == (0, 110)           # sparse: everything in between is staged
    t0, nt = U64(0), U64(0)
    assert L.uvdb_window_span(None, 5, 5, C.byref(t0), C.byref(nt), None) != 0       # an empty range is refused


def test_choose(L):
    bpr, free = 36000, 1 << 30                                           # 80 % of 1 GiB = 858 993 459 bytes = 23 860 references
    assert L.uvdb_window_choose(23860, 128, bpr, free) == 0               # fits: resident, as without --window
    assert L.uvdb_window_choose(0, 128, bpr, free) == 0
    for pool in (128, 96, 100, 4096):
        w = L.uvdb_window_choose(23861, pool, bpr, free)                 # one reference more does not
        assert w > 0
        assert _plan(L, 23861, pool, w)[:2] == (0, w)                     # a planned window: the plan leaves it as it is
        assert 3 * w * bpr <= free * 4 // 5                               # the window and two staging slots within the 80 %
        unit = _plan(L, 1, pool, 1)[1]
        assert 3 * (w + unit) * bpr > free * 4 // 5                       # and the largest such
    assert L.uvdb_window_choose(10 ** 9, 8192, bpr, free) < 0             # 3 x 8192 x 36 000 bytes are more than there is: an error value
    assert L.uvdb_window_choose(10, 64, bpr, 0) < 0


def test_new_abi_entries_are_exported_and_plain_c(tmp_path):
    capi.build_library()
    lib = capi.load_library()
    names = ("uvaia_gpu_db_stage_reserve", "uvaia_gpu_db_stage_packed", "uvaia_gpu_db_load_staged", "uvaia_gpu_db_unpack_rows", "uvaia_gpu_window_ms", "uvaia_gpu_free_bytes")
    for name in names:
        assert name in capi.SYMBOLS
        assert hasattr(lib, name), name
    for name in ("db_stage_reserve", "db_stage_packed", "db_load_staged", "db_unpack_rows", "window_ms", "free_bytes"):
        assert callable(getattr(capi.Engine, name))
    src = tmp_path / "t.c"
    src.write_text('#include "uvaia_gpu.h"\n'
                   "int (*reserve) (uvaia_gpu_ctx *, size_t) = uvaia_gpu_db_stage_reserve;\n"
                   "int (*stage) (uvaia_gpu_ctx *, int, const void *, const int *, const int *, int) = uvaia_gpu_db_stage_packed;\n"
                   "int (*load) (uvaia_gpu_ctx *, int, const int *, int) = uvaia_gpu_db_load_staged;\n"
                   "int (*text) (uvaia_gpu_ctx *, const int *, int, char *, size_t) = uvaia_gpu_db_unpack_rows;\n"
                   "void (*ms) (uvaia_gpu_ctx *, double *, int) = uvaia_gpu_window_ms;\n"
                   "size_t (*mem) (uvaia_gpu_ctx *) = uvaia_gpu_free_bytes;\n"
                   "int main (void) { return reserve == 0 || stage == 0 || load == 0 || text == 0 || ms == 0 || mem == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
    assert lib.uvaia_gpu_db_load_staged(None, 0, None, 0) == -1 and lib.uvaia_gpu_free_bytes(None) == 0      # no context: an error, not a fault


def test_uvaia_refuses_window_misuse_before_it_needs_a_gpu(tmp_path):
    """the checks of --window come before anything opens a GPU: a file written here (no GPU) is enough"""
    hostlib.build_library()
    uvaia = os.path.join(ROOT, "bin", "uvaia")
    nchar = 400
    root = F.random_acgt(nchar, 5)
    refs = [root] * 70
    planes, non_n = P.pack_tiles(refs, nchar)
    db = str(tmp_path / "r.uvdb")
    P.write_uvdb(db, ["r%d" % i for i in range(len(refs))], refs, planes, non_n, ref_ambiguity=0.5)
    q = tmp_path / "q.fa"
    q.write_bytes(b">q0\n" + root + b"\n>q1\n" + root[:10] + (b"A" if root[10:11] != b"A" else b"C") + root[11:] + b"\n")
    out = ["-o", str(tmp_path / "out")]
    for cmd in ([uvaia, "-r", str(q), "--window", "128", str(q)] + out,                          # without --packed
                [uvaia, "--packed", db, "--window", "0", str(q)] + out,                          # not positive
                [uvaia, "--packed", db, "--window=-5", str(q)] + out,
                [uvaia, "--packed", db, "--window", "many", str(q)] + out,
                [uvaia, "--packed", db, "--window", "128", "--devices", "0,1", str(q)] + out):   # several devices
        r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode != 0, cmd
        assert b"--window" in r.stderr, (cmd, r.stderr)
        assert b"HIP device" not in r.stderr, cmd            # refused on its own grounds, not for the missing GPU
        assert not os.path.exists(str(tmp_path / "out.csv.xz")), cmd
