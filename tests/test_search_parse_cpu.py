"""`uvaia -r --device-parse` and `uvaiaclust --device-parse` without a GPU: the window of resident references as a pure function of the host
library, and the option combinations that are refused while the options are read -- before a GPU is touched or a file created."""
import ctypes as C
import os
import subprocess

import pytest

from uvaia_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIA = os.path.join(ROOT, "bin", "uvaia")
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")
WINDOW_MAX = 0x7FFFFFFF - 63


def _window():
    L = hostlib.load_library()
    L.uvdb_parse_window.restype = C.c_uint64
    L.uvdb_parse_window.argtypes = [C.c_uint64] * 4
    return L.uvdb_parse_window


def test_the_window_is_whole_pools_within_half_of_the_free_memory():
    hostlib.build_library()
    w = _window()
    for pool in (1, 7, 64, 100, 4096, 65536, 100000):
        for nchar in (100, 29903):
            bpr = 3 * nchar + 300                                        # planes, derived planes and text of a reference, roughly
            for request in (0, 1, 64, 65536, 65537, 10 ** 6):
                asked = (request or 65536)
                rounded = (asked + pool - 1) // pool * pool
                last = 0
                for free in (1, 10 ** 6, 10 ** 8, 10 ** 9, 4 * 10 ** 9, 10 ** 10, 10 ** 11, 3 * 10 ** 11):
                    got = w(pool, request, bpr, free)
                    assert got % pool == 0 and got >= pool, (pool, nchar, request, free, got)
                    assert got <= rounded, (pool, nchar, request, free, got)
                    assert got == pool or got * bpr <= free // 2, (pool, nchar, request, free, got)      # lowered, but never below one pool
                    assert got >= last, (pool, nchar, request, free, got)                                # monotone in the free bytes
                    last = got
                assert w(pool, request, bpr, 0) == rounded               # free memory unknown: not lowered
                assert w(pool, request, bpr, 1 << 62) == rounded         # ... nor with memory to spare
    assert w(64, 0, 1000, 1 << 40) == 65536 and w(100, 0, 1000, 1 << 40) == 65600      # the default: the smallest multiple of the pool from 65 536 on
    assert w(64, 0, 1000, 2 * 1000 * 640) == 640 and w(64, 0, 1000, 2 * 1000 * 640 - 1) == 576
    assert w(0, 0, 1000, 1 << 40) == 0 and w(WINDOW_MAX + 1, 0, 1000, 1 << 40) == 0    # no pool, a pool beyond what the engine counts
    assert w(1000, 1 << 40, 1, 0) == WINDOW_MAX // 1000 * 1000


def _refused(cmd, option, outputs):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    text = (r.stdout + r.stderr).decode(errors="replace")
    assert r.returncode != 0, text
    assert option in text, text
    assert "HIP device" not in text and "Finished reading" not in text, text      # while the options are read: no GPU, no file
    for o in outputs:
        assert not os.path.exists(o), o


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    hostlib.build_library()
    d = tmp_path_factory.mktemp("search_parse_cpu")
    (d / "r.fa").write_bytes(b">r0\nACGTACGTAC\n>r1\nACGTACGTAA\n")
    (d / "q.fa").write_bytes(b">q0\nACGTACGTAC\n")
    (d / "db.uvdb").write_bytes(b"not a database")
    return d


def test_uvaia_refuses_what_does_not_go_with_the_option(inputs):
    d = inputs
    r, q, db, out = str(d / "r.fa"), str(d / "q.fa"), str(d / "db.uvdb"), str(d / "o")
    outputs = [out + ".aln.xz", out + ".csv.xz"]
    _refused([UVAIA, "--device-parse", "--packed", db, "-o", out, q], "--device-parse", outputs)
    _refused([UVAIA, "--device-parse", "--devices", "0,1", "-r", r, "-o", out, q], "--device-parse", outputs)
    _refused([UVAIA, "--parse-block", "4096", "-r", r, "-o", out, q], "--parse-block", outputs)
    _refused([UVAIA, "--parse-window", "64", "-r", r, "-o", out, q], "--parse-window", outputs)
    for block in ("63", "1073741825", "0"):
        _refused([UVAIA, "--device-parse", "--parse-block", block, "-r", r, "-o", out, q], "--parse-block", outputs)
    _refused([UVAIA, "--device-parse", "--parse-window", "0", "-r", r, "-o", out, q], "--parse-window", outputs)


def test_uvaiaclust_refuses_what_does_not_go_with_the_option(inputs):
    d = inputs
    r, db, out = str(d / "r.fa"), str(d / "db.uvdb"), str(d / "c")
    outputs = [out + ".aln.xz", out + ".csv.xz"]
    _refused([UVAIACLUST, "--device-parse", "--packed", db, "-o", out], "--device-parse", outputs)
    _refused([UVAIACLUST, "--parse-block", "4096", "-o", out, r], "--parse-block", outputs)
    for block in ("63", "1073741825"):
        _refused([UVAIACLUST, "--device-parse", "--parse-block", block, "-o", out, r], "--parse-block", outputs)
