"""Insertion runs of the wavefront aligner on the MI355X (`pytest -m gpu`): Aligner.insertions() against the table the oracle's CIGAR gives
(tests/align_insertions.py) record for record -- a run placed elsewhere inside a repeat leaves the same row and fails here --, through every
way a pool reaches the aligner, with a record buffer that is too small, over a second pass for workspace, with the option switched on and
off, and `uvaialign --insertions` through every output route."""
import ctypes as C
import lzma
import os
import subprocess

import numpy as np
import pytest

import align_edges as AE
import align_insertions as AI
import fixtures as F
import oracle_lib as O
from uvaia_amd import align, capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIALIGN = os.path.join(ROOT, "bin", "uvaialign")
ESTATE = -5


def _aligner(pool, **more):
    opts = dict(workspace_bytes=AE.WORKSPACE)
    opts.update(pool.opts)
    opts.update(more)
    return align.Aligner(pool.ref, **opts)


def _same(got, want, label):
    score, rows = got
    w_scores, w_rows = want
    assert score.tolist() == w_scores, label
    for i, r in enumerate(w_rows):
        assert rows[i].tobytes() == r, (label, i)


_hip = None


def _hip_runtime():
    """the HIP runtime the library itself is linked to, as this process has it loaded (tests/test_rows_gpu.py)"""
    global _hip
    if _hip is None:
        capi.load_library()
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        _hip = C.CDLL(path)
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


@pytest.mark.parametrize("name", AI.POOL_NAMES)
def test_records_equal_the_oracles_through_every_way_in(name):
    pool = AI.pool_named(name)
    seqs = list(pool.seqs)
    scores, rows, cells, table = AI.expected(pool)
    with _aligner(pool) as al:
        al.set_insertions(True)
        got = al.align(seqs)                                             # uvaia_align_batch
        _same(got, (scores, rows), (name, "align"))
        assert al.insertions() == table, (name, "align", al.insertions()[:4], table[:4])
        assert al.stats()["cells"] == cells and al.stats()["passes"] == 1
        al.load(seqs)                                                    # uvaia_align_load_block / run
        al.run()
        _same(al.fetch(), (scores, rows), (name, "load"))
        assert al.insertions() == table, (name, "load")
        blob = np.frombuffer(b"".join(seqs) + b"\0" * 64, dtype=np.uint8).copy()      # uvaia_align_load_device: the host keeps no text
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
        hip, base = _hip_runtime(), C.c_void_p()
        assert hip.hipMalloc(C.byref(base), blob.size) == 0
        try:
            assert hip.hipMemcpy(base, blob.ctypes.data, blob.size, 1) == 0
            al.load_device(base.value, off)
            blob[:] = 0
            al.run()
            _same(al.fetch(), (scores, rows), (name, "load_device"))
            assert al.insertions() == table, (name, "load_device")
        finally:
            hip.hipFree(base)


@pytest.mark.parametrize("capacity", [1, 4])
def test_a_record_buffer_that_is_too_small_grows_and_loses_nothing(capacity):
    pool = AI.many_runs_pool()
    scores, rows, cells, table = AI.expected(pool)
    assert len(table) == 20
    with _aligner(pool) as al:
        al.set_insertions(True, capacity)
        _same(al.align(list(pool.seqs)), (scores, rows), capacity)
        assert al.insertions() == table
        st = al.stats()
        assert st["passes"] == 2 and st["cells"] == cells, st
    # several queries, some of which fit the buffer before it fills: nothing doubled, nothing lost
    e = AI.pool_named("E")
    scores, rows, cells, table = AI.expected(e)
    with _aligner(e) as al:
        al.set_insertions(True, capacity)
        _same(al.align(list(e.seqs)), (scores, rows), ("E", capacity))
        assert al.insertions() == table
        assert al.stats()["passes"] >= 2 and al.stats()["cells"] == cells


def test_a_second_pass_for_workspace_leaves_every_record_once():
    """the shape of test_queries_that_find_the_pool_empty_are_run_again (tests/test_align_gpu.py)"""
    ref = F.random_acgt(6000, 17)
    seqs = F.unaligned_queries(ref, 24, 18, n_runs=(90, 75, 1200), run_prob=0.9)
    pool = AE.Pool("second-pass", ref, {}, tuple(seqs))
    scores, rows, cells, table = AI.expected(pool)
    assert len(table) >= 10
    with align.Aligner(ref, workspace_bytes=26 << 20, max_blocks=8) as al:
        al.set_insertions(True)
        _same(al.align(seqs), (scores, rows), "second pass")
        st = al.stats()
        assert st["passes"] >= 2 and st["cells"] == cells, st
        assert al.insertions() == table
        al.set_insertions(True, 2)                                       # both reasons to run a query again in one call
        _same(al.align(seqs), (scores, rows), "second pass, small buffer")
        assert al.insertions() == table and al.stats()["cells"] == cells


def test_off_before_a_run_and_switching():
    pool = AI.pool_named("I-leading")
    seqs = list(pool.seqs)
    scores, rows, cells, table = AI.expected(pool)
    with _aligner(pool) as al:
        with pytest.raises(align.AlignError) as e:                       # off, before a run
            al.insertions()
        assert e.value.code == ESTATE
        off = al.align(seqs)
        st_off = al.stats()
        with pytest.raises(align.AlignError) as e:                       # off, after a run
            al.insertions()
        assert e.value.code == ESTATE
        al.set_insertions(True)
        with pytest.raises(align.AlignError) as e:                       # on, before a run with the option on
            al.insertions()
        assert e.value.code == ESTATE
        al.load(seqs)
        with pytest.raises(align.AlignError) as e:                       # on, loaded, not run
            al.insertions()
        assert e.value.code == ESTATE
        al.run()
        on = al.fetch()
        st_on = al.stats()
        assert al.insertions() == table
        assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
        assert (st_on["cells"], st_on["passes"]) == (st_off["cells"], st_off["passes"]) == (cells, 1)
        al.set_insertions(False)
        again = al.align(seqs)
        assert np.array_equal(again[0], off[0]) and np.array_equal(again[1], off[1])
        with pytest.raises(align.AlignError) as e:
            al.insertions()
        assert e.value.code == ESTATE
        al.set_insertions(True)
        al.align(seqs[::-1])
        n = len(seqs)
        assert sorted((n - 1 - q, r, s, b) for q, r, s, b in al.insertions()) == table
        al.align([])                                                     # an empty pool has no runs
        assert al.insertions() == []


def test_rows_scores_cells_and_passes_do_not_depend_on_the_option():
    ref = F.random_acgt(3000, 61)
    seqs = F.unaligned_queries(ref, 64, 62, p_indel=0.004, n_runs=(20, 20, 60))
    with align.Aligner(ref, workspace_bytes=AE.WORKSPACE) as al:
        s0, r0 = (x.copy() for x in al.align(seqs))
        st0 = al.stats()
        al.set_insertions(True)
        s1, r1 = al.align(seqs)
        st1 = al.stats()
        table = al.insertions()
    assert np.array_equal(s0, s1) and np.array_equal(r0, r1)
    assert (st0["cells"], st0["passes"]) == (st1["cells"], st1["passes"])
    g_score, g_rows = O.uvaialign_batch(ref, seqs)
    assert np.array_equal(s1, g_score) and np.array_equal(r1, g_rows)
    assert len(table) > 20
    for q, seq in enumerate(seqs):
        assert AI.splice(r1[q].tobytes(), [(r, s, b) for qq, r, s, b in table if qq == q]) == seq, q


# ------------------------------------------------------------------------------------------------------------------ the command
VARIANTS = {"text": ["-o", "{stem}"], "stdout": ["--stdout"], "packed": ["--packed", "{stem}.uvdb"], "compact": ["--packed", "{stem}.c.uvdb", "--compact"],
            "parse": ["--device-parse", "-o", "{stem}"], "devices": ["--devices", "0,0", "-o", "{stem}"]}


@pytest.fixture(scope="module")
def commands(tmp_path_factory):
    d = tmp_path_factory.mktemp("align_insertions")
    ref, names, seqs, dropped = AI.cli_case()
    (d / "ref.fa").write_bytes(b">the reference\n" + ref + b"\n")
    (d / "in.fa").write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in zip(names, seqs)))
    res = {}
    for with_table in (False, True):                                     # six commands at a time
        procs = {}
        for how, args in VARIANTS.items():
            stem = str(d / ("%s.%s" % (how, "ins" if with_table else "plain")))
            table = stem + (".csv.xz" if how == "text" else ".csv")
            cmd = [UVAIALIGN, "-r", str(d / "ref.fa"), "-p", "5", "-A", AI.CLI_AMBIG_R] + [a.format(stem=stem) for a in args] + (["--insertions", table] if with_table else []) + [str(d / "in.fa")]
            procs[how] = (subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE), stem, table)
        try:
            for how, (p, stem, table) in procs.items():
                out, err = p.communicate(timeout=300)
                res[(how, with_table)] = (p.returncode, out, err.decode(errors="replace"), stem, table)
        finally:
            for p, _, _ in procs.values():
                if p.poll() is None:
                    p.kill()
                    p.communicate()
        died = [(k, r[0]) for k, r in res.items() if r[0] != 0]
        assert not died, (died, [res[k][2][-1500:] for k, _ in died[:1]])
    return d, res, AI.cli_table(ref, names, seqs, dropped), dropped


@pytest.mark.parametrize("how", list(VARIANTS))
def test_the_table_is_the_oracles_whatever_the_route(commands, how):
    d, res, want, dropped = commands
    rc, out, err, stem, table = res[(how, True)]
    got = lzma.open(table, "rb").read() if table.endswith(".xz") else open(table, "rb").read()
    assert got == want
    assert "Insertions: 10 sequences with insertions, %d inserted bases" % sum(len(ln.split(b",")[-1]) for ln in want.split(b"\n")[1:-1]) in err, err[-1500:]
    assert "Insertions" not in res[(how, False)][2]
    for name in dropped:
        assert "Sequence %s has size too different" % name in err


@pytest.mark.parametrize("how", list(VARIANTS))
def test_the_other_outputs_do_not_change(commands, how):
    d, res, want, dropped = commands
    plain, ins = res[(how, False)], res[(how, True)]
    base = lzma.open(res[("text", False)][3] + ".aln.xz", "rb").read()
    assert base.count(b">") == 12
    if how == "stdout":
        assert plain[1] == ins[1] == base
    elif how in ("packed", "compact"):
        suffix = ".uvdb" if how == "packed" else ".c.uvdb"
        a, b = open(plain[3] + suffix, "rb").read(), open(ins[3] + suffix, "rb").read()
        assert a == b and len(a) > 1024
        assert "Packed 11 of 12 aligned sequences" in ins[2] and "; 1 too ambiguous" in ins[2], ins[2][-1500:]      # the twelfth is listed all the same
    else:
        assert lzma.open(plain[3] + ".aln.xz", "rb").read() == lzma.open(ins[3] + ".aln.xz", "rb").read() == base
