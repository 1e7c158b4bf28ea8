"""Rows that are already in device memory on their way into the packed database, on a GPU box: the census and the exception records against
the host rules, uvaia_gpu_db_append_device against uvaia_gpu_db_append (same planes, counts, side rows, heaps), the refusals, and the rows the
aligner hands out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures as F
import oracle_lib as O
import rows_lib as R
from uvaia_amd import align, capi

pytestmark = pytest.mark.gpu


def _query(nchar, acgt=False, nq=5, seed=3):
    root = F.random_acgt(nchar, seed)
    qs = []
    for i in range(nq):
        s = bytearray(root)
        for k in range(1 + i):
            at = (131 * i + 17 * k + 3) % nchar
            s[at] = b"ACGT"[(b"ACGT".index(s[at]) + 1 + k) % 4]
        qs.append(bytes(s))
    return O.Query(qs, ["q%d" % i for i in range(nq)], acgt=acgt)


_hip = None


def _hip_runtime():
    """the HIP runtime the engine library itself is linked to, as this process has it loaded (a second runtime next to it -- the one a torch
    wheel brings along -- does not find the GPU once this one holds it: the torch tensor has a test of its own, in a fresh process)"""
    global _hip
    if _hip is None:
        capi.load_library()
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        _hip = C.CDLL(path)
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


class DeviceBlock:
    """rows in device memory, `shift` bytes into their allocation; the bytes between and around the rows are 'U', which the engine refuses
    wherever it reads it"""

    def __init__(self, rows, nchar, pitch, shift):
        hip = _hip_runtime()
        self.n, self.pitch = len(rows), pitch
        host = np.full(shift + self.n * pitch + 64, ord("U"), dtype=np.uint8)
        body = host[shift:shift + self.n * pitch].reshape(self.n, pitch)
        for i, r in enumerate(rows):
            body[i, :nchar] = np.frombuffer(r, dtype=np.uint8)
        self.base = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.base), host.size) == 0
        assert hip.hipMemcpy(self.base, host.ctypes.data, host.size, 1) == 0          # hipMemcpyHostToDevice
        self.ptr = self.base.value + shift

    def args(self, n=None):
        return dict(pitch=self.pitch, n=self.n if n is None else n)

    def __del__(self):
        if self.base:
            _hip_runtime().hipFree(self.base)
            self.base = None


def _device_block(rows, nchar, pitch, shift):
    return DeviceBlock(rows, nchar, pitch, shift), None


def _export_and_heaps(eng, pool=64):
    out = eng.db_export() if not eng_acgt(eng) else None
    eng.reset()
    eng.search_resident(pool)
    n, T, sc, od = eng.drain()
    return out, (n.copy(), T.copy(), sc.copy(), od.copy())


def eng_acgt(eng):
    return getattr(eng, "_acgt", False)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("nchar,shift", [(1237, 5), (2048, 0), (29903, 3)])
@pytest.mark.parametrize("acgt", [False, True])
def test_db_append_device_leaves_what_db_append_leaves(nchar, shift, acgt):
    n = 150 if nchar < 10000 else 90
    rows = R.random_rows(n, nchar, seed=nchar, special=True)
    pitch = nchar + 14 if (nchar + 14) % 2 else nchar + 15            # odd and larger than nchar
    rng = np.random.default_rng(7)
    index = [int(x) for x in rng.permutation(n)[:n - 23]]               # skips rows and reorders them
    q = _query(nchar, acgt)
    t, _keep = _device_block(rows, nchar, pitch, shift)
    results = []
    for how in ("host", "device", "device_counts", "device_split", "device_all_then_drop"):
        with capi.Engine.from_query(q, nbest=4, max_pool=64) as eng:
            eng._acgt = acgt
            eng.db_reserve(2 * n)
            if how == "host":
                eng.db_append([rows[i] for i in index])
            elif how == "device":
                eng.db_append_device(t.ptr, row_index=index, **t.args())
            elif how == "device_counts":
                eng.db_append_device(t.ptr, **t.args(), row_index=index, non_n=[R.count_non_n(rows[i]) for i in index])
            elif how == "device_split":                                  # two calls that split inside a tile
                eng.db_append_device(t.ptr, row_index=index[:37], **t.args())
                eng.db_append_device(t.ptr, row_index=index[37:], pitch=pitch)
            else:                                                        # every row in order (row_index NULL), then the wanted ones behind: drop the first tiles
                eng.db_append_device(t.ptr, **t.args(64))
                eng.db_append_device(t.ptr, row_index=index, **t.args())
                eng.db_drop_tiles(1)
            assert eng.db_size() == len(index)
            results.append(_export_and_heaps(eng))
    want_export, want_heaps = results[0]
    for how, (export, heaps) in zip(("device", "device_counts", "device_split", "device_all_then_drop"), results[1:]):
        if not acgt:
            assert np.array_equal(export[0], want_export[0]), (how, "planes")
            assert np.array_equal(export[1], want_export[1]), (how, "valid-site counts")
            assert np.array_equal(export[2], want_export[2]), (how, "side rows")
        assert _same(heaps, want_heaps), (how, "heaps")
    assert int(want_heaps[0].sum()) > 0
    if not acgt:                                                         # side rows in their fixed form: ascending words, the first eleven of them
        side = want_export[2].reshape(-1, 64)[:len(index)]
        assert int((side[:, 0] > 11).sum()) > 0
        for row in side:
            listed = list(row[1:1 + min(int(row[0]), 11)])
            assert listed == sorted(set(listed)), listed


@pytest.mark.parametrize("nchar,shift,pitch_extra", [(29903, 0, 1), (29903, 7, 0), (1237, 1, 6), (16, 0, 0), (5, 2, 3)])
def test_census_and_exception_records_follow_the_host_rules(nchar, shift, pitch_extra):
    n = 40
    rows = R.random_rows(n, nchar, seed=100 + nchar, special=nchar > 100)
    if nchar <= 100:
        rows = [bytes(np.random.default_rng(i).choice(np.frombuffer(b"ACGT-?XO.Nnxo", dtype=np.uint8), size=nchar)) for i in range(n)]
        rows[0], rows[1] = b"-" * nchar, b"ACGT" * (nchar // 4) + b"A" * (nchar % 4)
    t, _keep = _device_block(rows, nchar, nchar + pitch_extra, shift)
    with capi.Engine.from_query(_query(nchar), nbest=2, max_pool=64) as eng:
        non_n, n_exc = eng.rows_census(t.ptr, **t.args())
        want = [R.exception_runs(r) for r in rows]
        assert list(non_n) == [R.count_non_n(r) for r in rows]
        assert list(n_exc) == [len(w) for w in want]
        assert non_n[0] == 0 and n_exc[0] == 1 and non_n[1] == nchar and n_exc[1] == 0      # all '-' and all ACGT
        off, rec = eng.rows_exceptions(t.ptr, n_exc, **t.args())
        assert [tuple(int(v) for v in x) for x in rec] == [x for w in want for x in w]
        index = [int(x) for x in np.random.default_rng(1).permutation(n)[:n - 9]]
        off, rec = eng.rows_exceptions(t.ptr, [n_exc[i] for i in index], row_index=index, **t.args())
        for k, i in enumerate(index):
            assert [tuple(int(v) for v in x) for x in rec[int(off[k]):int(off[k + 1])]] == want[i], i
        # the cut of long runs, reached with short rows: same rule, other length
        for cut in (1, 7, 4096):
            eng.rows_set_run_cut(cut)
            want_c = [R.exception_runs(r, cut=cut) for r in rows]
            non_n_c, n_exc_c = eng.rows_census(t.ptr, **t.args())
            assert list(non_n_c) == list(non_n) and list(n_exc_c) == [len(w) for w in want_c], cut
            off, rec = eng.rows_exceptions(t.ptr, n_exc_c, **t.args())
            assert [tuple(int(v) for v in x) for x in rec] == [x for w in want_c for x in w], cut
        eng.rows_set_run_cut(0)
        assert list(eng.rows_census(t.ptr, **t.args())[1]) == [len(w) for w in want]
        ms = eng.rows_kernel_ms()
        assert ms["census"] > 0 and ms["exceptions"] > 0


def test_bad_bytes_and_bad_pointers_are_error_codes():
    nchar, n = 777, 20
    rows = R.random_rows(n, nchar, seed=4)
    bad = list(rows)
    bad[11] = bad[11][:500] + b"U" + bad[11][501:]
    t, _k1 = _device_block(rows, nchar, nchar + 3, 1)
    tb, _k2 = _device_block(bad, nchar, nchar + 3, 1)
    with capi.Engine.from_query(_query(nchar), nbest=2, max_pool=64) as eng:
        with pytest.raises(capi.GpuError) as ei:
            eng.rows_census(tb.ptr, **tb.args())
        assert ei.value.code == -5                                       # UVAIA_GPU_EALPHABET, as uvaia_gpu_db_append
        with pytest.raises(capi.GpuError) as ei:
            eng.db_append_device(tb.ptr, **tb.args())
        assert ei.value.code == -5
        host = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
        for call in (lambda: eng.rows_census(host.ctypes.data, pitch=nchar, n=n),                         # host memory
                     lambda: eng.db_append_device(host.ctypes.data, pitch=nchar, n=n),
                     lambda: eng.rows_census(t.ptr, pitch=nchar + 3, n=1 << 24),                    # rows beyond the allocation
                     lambda: eng.db_append_device(t.ptr, row_index=[0, 1 << 24], **t.args()),
                     lambda: eng.db_append_device(t.ptr, row_index=[3, -1], **t.args()),
                     lambda: eng.rows_census(t.ptr, pitch=nchar - 1, n=n),                          # pitch below a row
                     lambda: eng.rows_exceptions(t.ptr, [0] * n, **t.args())):                                              # offsets that are not these rows'
            with pytest.raises(capi.GpuError) as ei:
                call()
            assert ei.value.code == -1                                   # UVAIA_GPU_EINVAL
        non_n, n_exc = eng.rows_census(t.ptr, **t.args())                                # ... and the context is still usable
        assert list(non_n) == [R.count_non_n(r) for r in rows]
        assert eng.db_size() == 0


def test_rows_of_the_aligner_go_into_the_database_where_they_lie():
    ref = F.random_acgt(1501, 3)
    seqs = F.unaligned_queries(ref, 70, 4, n_runs=(20, 20, 60))
    with align.Aligner(ref) as al:
        al.load(seqs)
        with pytest.raises(align.AlignError) as ei:
            al.device_rows()
        assert ei.value.code == -5                                       # UVAIA_ALIGN_ESTATE: no completed run
        al.run()
        ptr, pitch, n, dev = al.device_rows()
        assert ptr and pitch == len(ref) + 1 and n == len(seqs) and dev == 0
        _score, fetched = al.fetch()
        text = [bytes(r) for r in fetched]
        q = _query(len(ref))
        with capi.Engine.from_query(q, nbest=3, max_pool=64) as eng:
            non_n, n_exc = eng.rows_census(ptr, pitch=pitch, n=n)
            assert list(non_n) == [R.count_non_n(r) for r in text]
            assert list(n_exc) == [len(R.exception_runs(r)) for r in text]
            assert int(n_exc.sum()) > 0                                  # the deletions are there
            eng.db_append_device(ptr, pitch=pitch, n=n, non_n=non_n)
            got = eng.db_export()
        with capi.Engine.from_query(q, nbest=3, max_pool=64) as eng:
            eng.db_append(text, non_n=non_n)
            want = eng.db_export()
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


TORCH_WORKER = r"""
import sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, root + "/tests")
import numpy as np
import torch
torch.cuda.init()                                     # the tensor's runtime first, the engine's after it
import rows_lib as R
import test_rows_gpu as T
from uvaia_amd import capi
nchar, n, pitch = 1237, 100, 1251
rows = R.random_rows(n, nchar, seed=1)
host = np.full((n, pitch), ord("U"), dtype=np.uint8)
for i, r in enumerate(rows):
    host[i, :nchar] = np.frombuffer(r, dtype=np.uint8)
wide = torch.from_numpy(host).cuda()
index = [int(x) for x in np.random.default_rng(2).permutation(n)[:70]]
q = T._query(nchar)
with capi.Engine.from_query(q, nbest=3, max_pool=64) as eng:
    non_n, n_exc = eng.rows_census(wide)
    assert list(non_n) == [R.count_non_n(r) for r in rows]
    off, rec = eng.rows_exceptions(wide[:, :nchar + 3], n_exc)          # a view: rows contiguous, row stride the wide tensor's
    assert [tuple(int(v) for v in x) for x in rec] == [x for r in rows for x in R.exception_runs(r)]
    eng.db_append_device(wide, row_index=index)
    got = eng.db_export()
    try:
        eng.db_append_device(wide.cpu())
        raise SystemExit("a host tensor was accepted")
    except capi.GpuError as e:
        assert e.code == -1
with capi.Engine.from_query(q, nbest=3, max_pool=64) as eng:
    eng.db_append([rows[i] for i in index])
    want = eng.db_export()
assert all(np.array_equal(a, b) for a, b in zip(got, want))
print("TENSOR OK")
"""


def test_a_torch_tensor_goes_into_the_database_without_a_copy(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(TORCH_WORKER)
    r = subprocess.run([sys.executable, str(script), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"TENSOR OK" in r.stdout, r.stderr[-3000:]
