"""Host-side pieces of `uvaiaclust --keep-medoids` that need no GPU: the rule that chooses the mode for a packed database
(uvaia_amd/csrc/host/clust_plan.h) and the new entries of include/uvaia_cluster.h (plain C, exported)."""
import ctypes as C
import os
import subprocess

import pytest

from uvaia_amd import capi, cluster, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = C.c_uint64
ROW = 29952                      # a 29 903-site genome at the 64-byte pitch of the row store
HBM = 288 * 10 ** 9


@pytest.fixture(scope="module")
def L():
    hostlib.build_library()
    lib = hostlib.load_library()
    lib.uvclust_store_peak.restype = C.c_int
    lib.uvclust_store_peak.argtypes = [U64, U64, U64, C.POINTER(U64)]
    lib.uvclust_choose_keep_medoids.restype = C.c_int
    lib.uvclust_choose_keep_medoids.argtypes = [U64, U64, U64, U64]
    return lib


def schedule_peak_rows(n_rows, push_rows):
    """the schedule clust_plan.h documents, push by push: capacity 0, raised to max(needed, 2 x capacity, 1024); a step holds old + new"""
    cap = peak = pushed = 0
    while pushed < n_rows:
        need = pushed + min(push_rows, n_rows - pushed)
        if need > cap:
            to = max(need, 2 * cap, 1024)
            peak = max(peak, cap + to)
            cap = to
        pushed = need
    return peak


def _peak(L, n, push, row):
    out = U64(0)
    assert L.uvclust_store_peak(n, push, row, C.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("n,push", [(n, push) for push in (1, 64, 256, 1000, 4096) for n in (0, 1, 1023, 1024, 1025, 4096, 4097, 70000, 262144, 262145)
                                    if n // push <= 100000])                      # (the push-by-push replay in Python of the rest is slow)
def test_store_peak_is_the_documented_schedule(L, n, push):
    assert _peak(L, n, push, 7) == 7 * schedule_peak_rows(n, push)


def test_a_count_that_fits_keeps_every_row_and_a_step_that_does_not_fit_keeps_medoids(L):
    # pushes of 4 096: capacities 4 096, 8 192, 16 384; the step to 16 384 holds 8 192 + 16 384 rows
    assert _peak(L, 8192, 4096, 100) == (4096 + 8192) * 100
    assert _peak(L, 8193, 4096, 100) == (8192 + 16384) * 100
    free = (8192 + 16384) * 100
    assert L.uvclust_choose_keep_medoids(8193, 4096, 100, free) == 0              # just fits
    assert L.uvclust_choose_keep_medoids(8193, 4096, 100, free - 1) == 1          # the doubling step does not, although 8 193 rows would
    assert 8193 * 100 < free - 1
    assert L.uvclust_choose_keep_medoids(8192, 4096, 100, free - 1) == 0
    assert L.uvclust_choose_keep_medoids(0, 4096, 100, 1) == 0


def test_the_ceiling_of_a_288_gb_device(L):
    assert _peak(L, 4194304, 4096, ROW) == (2097152 + 4194304) * ROW == ROW * schedule_peak_rows(4194304, 4096)
    assert _peak(L, 4194305, 4096, ROW) == (4194304 + 8388608) * ROW == ROW * schedule_peak_rows(4194305, 4096)
    assert (2097152 + 4194304) * ROW < HBM < (4194304 + 8388608) * ROW            # 188 GB and 377 GB
    assert L.uvclust_choose_keep_medoids(4194304, 4096, ROW, HBM) == 0
    assert L.uvclust_choose_keep_medoids(4194305, 4096, ROW, HBM) == 1
    assert L.uvclust_choose_keep_medoids(10 ** 7, 4096, ROW, HBM) == 1            # the 10 M-reference database


def test_unknown_free_memory_keeps_every_row(L):
    assert L.uvclust_choose_keep_medoids(10 ** 7, 4096, ROW, 0) == 0
    assert L.uvclust_choose_keep_medoids(1 << 62, 4096, ROW, 0) == 0


def test_plan_refuses_what_it_cannot_count_and_saturates(L):
    assert L.uvclust_choose_keep_medoids(10, 0, ROW, HBM) == -1
    assert L.uvclust_choose_keep_medoids(10, 4096, 0, HBM) == -1
    assert L.uvclust_store_peak(10, 4096, ROW, None) == 0                          # the output is nullable
    assert _peak(L, 1 << 62, 1 << 61, 1 << 20) == 2 ** 64 - 1
    assert L.uvclust_choose_keep_medoids(1 << 62, 1 << 61, 1 << 20, HBM) == 1


def test_new_abi_entries_are_exported_and_plain_c(tmp_path):
    capi.build_library()
    lib = capi.load_library()
    for name in ("uvaia_clust_keep_medoids", "uvaia_clust_gather_device", "uvaia_clust_memory"):
        assert name in cluster.SYMBOLS
        assert hasattr(lib, name), name
    for name in ("keep_medoids", "gather_device", "memory", "device_rows"):
        assert callable(getattr(cluster.Clusterer, name))
    src = tmp_path / "t.c"
    src.write_text('#include "uvaia_cluster.h"\n'
                   "int (*keep) (uvaia_clust_ctx *, int) = uvaia_clust_keep_medoids;\n"
                   "int (*gather) (uvaia_clust_ctx *, const int64_t *, int, const void **, size_t *) = uvaia_clust_gather_device;\n"
                   "int (*mem) (uvaia_clust_ctx *, size_t *, size_t *, size_t *) = uvaia_clust_memory;\n"
                   "int main (void) { return keep == 0 || gather == 0 || mem == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
    cluster._lib()
    assert lib.uvaia_clust_keep_medoids(None, 0) == -1 and lib.uvaia_clust_memory(None, None, None, None) == -1      # no context: an error, not a fault
    assert lib.uvaia_clust_gather_device(None, None, 0, None, None) == -1


def test_host_library_exports_the_plan_and_its_header_is_plain_c(L, tmp_path):
    assert hasattr(L, "uvclust_store_peak") and hasattr(L, "uvclust_choose_keep_medoids")
    src = tmp_path / "t.c"
    src.write_text('#include "clust_plan.h"\n'
                   "int (*choose) (uint64_t, uint64_t, uint64_t, uint64_t) = uvclust_choose_keep_medoids;\n"
                   "int (*peak) (uint64_t, uint64_t, uint64_t, uint64_t *) = uvclust_store_peak;\n"
                   "int main (void) { return choose == 0 || peak == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "uvaia_amd", "csrc", "host"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_cli_help_names_the_option():
    hostlib.build_library()
    r = subprocess.run([os.path.join(ROOT, "bin", "uvaiaclust"), "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--keep-medoids" in r.stdout
