"""The text row store (uvaia_gpu_text_*, include/uvaia_gpu.h) on a GPU box: rows appended from device memory of any pitch and alignment
come back as they went in, in any order and with repeats; the store grows and keeps its content; every refusal leaves it as it was."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_rows_gpu import DeviceBlock
from uvaia_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 0xEE
ALPHABET = np.frombuffer(b"ACGTacgtMRWSYKVHDBmrwsykvhdbNnXxOo-?.", dtype=np.uint8)


def _round16(x):
    return (x + 15) // 16 * 16


def _engine(nchar, acgt):
    """a context for rows of nchar sites, down to one: the query every command without queries of its own opens the engine with, a plain
    ACGT string and no column lists (the oracle's preparation keeps no query of fewer than four sites)"""
    dummy = bytes(b"ACGT"[s & 3] for s in range(nchar))
    return capi.Engine([dummy], dummy, [], [], [], acgt=acgt, nbest=2, max_pool=64)


def _rows(n, nchar, seed):
    rng = np.random.default_rng(seed)
    return [rng.choice(ALPHABET, size=nchar).tobytes() for _ in range(n)]


def _selections(n):
    """none, every second, reversed, one row repeated"""
    return [None, list(range(0, n, 2)), list(range(n - 1, -1, -1)), [n // 2] * 3]


def _fetch(eng, index, host_pitch):
    """text_rows into a guarded buffer: (rows [m, nchar], the bytes the call must not have written)"""
    m = len(index)
    buf = np.full(m * host_pitch + 64, GUARD, dtype=np.uint8)
    out = buf[:m * host_pitch].reshape(m, host_pitch)
    eng.text_rows(index, pitch=host_pitch, out=out)
    untouched = [buf[m * host_pitch:]]
    if host_pitch != _round16(eng.nchar):              # behind nchar only the rounded pitch may be written
        untouched.append(out[:, eng.nchar:])
    return out[:, :eng.nchar], untouched


@pytest.mark.parametrize("acgt", [False, True])
@pytest.mark.parametrize("nchar", [1, 15, 16, 17, 33, 4099])
def test_rows_come_back_as_they_went_in(nchar, acgt):
    n = 9
    rows = _rows(n, nchar, seed=nchar)
    want_rows = np.stack([np.frombuffer(r, dtype=np.uint8) for r in rows])
    sels = _selections(n)
    host_pitches = [nchar, nchar + 1, _round16(nchar)]
    rng = np.random.default_rng(nchar + 1)
    case = 0
    with _engine(nchar, acgt) as eng:
        for pitch in (nchar, nchar + 5, _round16(nchar)):        # rows back to back, an odd pitch, the store's own
            for shift in range(16):
                block = DeviceBlock(rows, nchar, pitch, shift)
                eng.text_clear()
                expect = []
                for a in range(3):                               # three appends in a row
                    sel = sels[(case + a) % 4]
                    eng.text_append_device(block.ptr, row_index=sel, **block.args())
                    expect += list(range(n)) if sel is None else sel
                    assert eng.text_size() == len(expect)
                size = len(expect)
                for index in (list(range(size)), [int(x) for x in rng.integers(0, size, size=size + 7)]):      # in order; any order, with repeats
                    got, untouched = _fetch(eng, index, host_pitches[case % 3])
                    assert np.array_equal(got, want_rows[[expect[i] for i in index]]), (pitch, shift, case)
                    assert all((u == GUARD).all() for u in untouched), (pitch, shift, case)
                case += 1
        ms = eng.text_ms()
        assert ms["in"] > 0 and ms["out"] > 0


@pytest.mark.parametrize("acgt", [False, True])
def test_the_store_grows_and_keeps_its_rows(acgt):
    nchar, n = 133, 5
    rows = _rows(n, nchar, seed=2)
    block = DeviceBlock(rows, nchar, nchar + 3, 7)
    with _engine(nchar, acgt) as eng:
        eng.text_reserve(2)
        eng.text_append_device(block.ptr, pitch=block.pitch, n=2)
        eng.text_append_device(block.ptr, row_index=[2, 3, 4], **block.args())      # beyond the two rows reserved
        assert eng.text_size() == 5
        got, _u = _fetch(eng, [0, 1, 2, 3, 4], nchar)
        assert [bytes(r) for r in got] == rows
        eng.text_clear()
        assert eng.text_size() == 0
        with pytest.raises(capi.GpuError) as ei:
            eng.text_rows([0])                                    # nothing is left to hand out
        assert ei.value.code == -1
        eng.text_append_device(block.ptr, row_index=[4, 0], **block.args())
        got, _u = _fetch(eng, [1, 0], nchar)
        assert [bytes(r) for r in got] == [rows[0], rows[4]]


@pytest.mark.parametrize("acgt", [False, True])
def test_refusals_leave_the_store_as_it_was(acgt):
    nchar, n = 777, 6
    rows = _rows(n, nchar, seed=4)
    block = DeviceBlock(rows, nchar, nchar + 3, 1)
    host = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    with _engine(nchar, acgt) as eng:
        eng.text_append_device(block.ptr, row_index=[5, 1, 3], **block.args())
        out = np.full((4, nchar + 2), GUARD, dtype=np.uint8)
        pi = C.POINTER(C.c_int)
        one = (C.c_int * 1)(0)
        for call in (lambda: eng.text_append_device(host.ctypes.data, pitch=nchar, n=n),                  # host memory
                     lambda: eng.text_append_device(block.ptr, pitch=nchar + 3, n=1 << 24),              # rows beyond the allocation
                     lambda: eng.text_append_device(block.ptr, row_index=[0, 1 << 24], **block.args()),
                     lambda: eng.text_append_device(block.ptr, row_index=[3, -1], **block.args()),       # a negative row
                     lambda: eng.text_append_device(block.ptr, pitch=nchar - 1, n=n),                    # pitch below a row
                     lambda: eng._chk(eng.L.uvaia_gpu_text_append_device(eng.ctx, block.ptr, nchar + 3, None, -1)),      # a negative count
                     lambda: eng.text_rows([0, 3], pitch=nchar + 2, out=out),                            # index at the store size
                     lambda: eng.text_rows([-1], pitch=nchar + 2, out=out),
                     lambda: eng.text_rows([0, 1], pitch=nchar - 1, out=out),                            # pitch below a row
                     lambda: eng._chk(eng.L.uvaia_gpu_text_rows(eng.ctx, C.cast(one, pi), -1, out.ctypes.data, nchar + 2))):
            with pytest.raises(capi.GpuError) as ei:
                call()
            assert ei.value.code == -1                                   # UVAIA_GPU_EINVAL
            assert eng.text_size() == 3
            assert (out == GUARD).all()                                  # nothing was copied
        got, _u = _fetch(eng, [0, 1, 2], nchar)                          # ... the content is what it was and the context is usable
        assert [bytes(r) for r in got] == [rows[5], rows[1], rows[3]]
        eng.text_append_device(block.ptr, row_index=[0], **block.args())
        got, _u = _fetch(eng, [3], nchar + 1)
        assert bytes(got[0]) == rows[0]
        assert eng.db_size() == 0                                        # the store stands next to the resident database, not in it


TORCH_WORKER = r"""
import sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, root + "/tests")
import numpy as np
import torch
torch.cuda.init()                                     # the tensor's runtime first, the engine's after it
import test_rows_gpu as T
from uvaia_amd import capi
nchar, n, pitch = 1237, 40, 1251
rng = np.random.default_rng(1)
host = rng.choice(np.frombuffer(b"ACGTNacgtn-?.XORYKM", dtype=np.uint8), size=(n, pitch))
wide = torch.from_numpy(host).cuda()
index = [int(x) for x in rng.permutation(n)[:25]]
for acgt in (False, True):
    with capi.Engine.from_query(T._query(nchar, acgt), nbest=3, max_pool=64) as eng:
        eng.text_append_device(wide)                                     # every row of the wide tensor
        eng.text_append_device(wide[:, 3:nchar + 3], row_index=index)    # a view: rows contiguous and misaligned, row stride the wide tensor's
        assert eng.text_size() == n + len(index)
        got = eng.text_rows(list(range(n + len(index))))
        assert np.array_equal(got[:n], host[:, :nchar]) and np.array_equal(got[n:], host[index, 3:nchar + 3])
        try:
            eng.text_append_device(wide.cpu())
            raise SystemExit("a host tensor was accepted")
        except capi.GpuError as e:
            assert e.code == -1 and eng.text_size() == n + len(index)
print("TENSOR OK")
"""


def test_a_torch_tensor_goes_into_the_store(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(TORCH_WORKER)
    r = subprocess.run([sys.executable, str(script), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"TENSOR OK" in r.stdout, r.stderr[-3000:]
