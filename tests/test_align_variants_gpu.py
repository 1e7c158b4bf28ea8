"""Substitutions, deletions and per-row counts of the wavefront aligner's rows on the MI355X (`pytest -m gpu`): Aligner.variants_of and
Aligner.variants against the numpy restatement of the specification (tests/align_variants.py), record for record and count for count -- at
the lane, round and row edges of the kernels' walk with every row alignment, over more rows than the offset scan's block has threads,
through every way a pool reaches the aligner with the insertion records on and off --, the state the entries keep and refuse in, and
`uvaialign --variants --qc` through every output route."""
import ctypes as C
import gzip
import lzma
import os
import subprocess

import numpy as np
import pytest

import align_edges as AE
import align_insertions as AI
import align_variants as AV
from uvaia_amd import align, capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIALIGN = os.path.join(ROOT, "bin", "uvaialign")
EINVAL, ESTATE = -1, -5


def _aligner(pool, **more):
    opts = dict(workspace_bytes=AE.WORKSPACE)
    opts.update(pool.opts)
    opts.update(more)
    return align.Aligner(pool.ref, **opts)


def _equal(got, want, label):
    """(records, qc) of the device against restate()'s, everything"""
    rec, qc = got
    w_rec, w_qc = want
    assert AV.counts_of(qc) == [tuple(q) for q in w_qc], (label, "counts")
    g_rec = AV.records_of(rec)
    assert len(g_rec) == len(w_rec), (label, len(g_rec), len(w_rec))
    assert g_rec == w_rec, (label, next((g, w) for g, w in zip(g_rec, w_rec) if g != w))
    assert not rec["pad"].any(), label


# ------------------------------------------------------------------------------------------------------------------ edges of the walk
@pytest.fixture(scope="module")
def edges():
    names, rows = AV.edge_rows()
    return rows, AV.restate(rows, AV.edge_ref()), AV.restate(rows, AV.edge_ref_with_n())


@pytest.mark.parametrize("pitch", AV.EDGE_PITCHES)
def test_edges_with_every_row_alignment(edges, pitch):
    rows, want, want_n = edges
    if pitch % 2:
        assert {(i * pitch) % 16 for i in range(len(rows))} == set(range(16))           # every start residue occurs
    buf = AV.flat(rows, pitch)
    with align.Aligner(AV.edge_ref()) as al:
        _equal(al.variants_of(buf, pitch), want, pitch)
        assert al.variants_ms() > 0
        if pitch == AV.EDGE_LEN:
            _equal(al.variants_of(rows), want, "a list of rows")
            _equal(al.variants_of(np.frombuffer(buf, dtype=np.uint8).reshape(len(rows), pitch)), want, "a 2-D array")
    with align.Aligner(AV.edge_ref_with_n()) as al:                                       # a base opposite a reference byte N
        _equal(al.variants_of(buf, pitch), want_n, (pitch, "N in the reference"))


def test_a_row_order_that_moves_every_row_to_another_residue(edges):
    rows, _, _ = edges
    rows = rows[::-1] + rows[5:9]
    want = AV.restate(rows, AV.edge_ref())
    with align.Aligner(AV.edge_ref()) as al:
        _equal(al.variants_of(AV.flat(rows, AV.EDGE_LEN + 1, pad=b"A"), AV.EDGE_LEN + 1), want, "reversed")


# ------------------------------------------------------------------------------------------------------------------ the offsets
def test_offsets_over_more_rows_than_a_block_has_threads():
    ref, rows = AV.offsets_case()
    want = AV.restate(rows, ref)
    with align.Aligner(ref) as al:
        _equal(al.variants_of(rows), want, "2100 rows")
        _equal(al.variants_of(AV.flat(rows, 41), 41), want, "2100 rows, pitch 41")
        for a, b in ((1, 2), (0, 1), (2, 3), (0, 0), (0, 1025), (3, 1028)):              # n = 1 with and without records, n = 0, one row past the block
            _equal(al.variants_of(rows[a:b]), AV.restate(rows[a:b], ref), (a, b))
        rec, qc = al.variants_of([])
        assert rec.size == 0 and qc.size == 0
        _equal(al.variants_of(rows), want, "after an empty call")


@pytest.mark.parametrize("ref_len", [7, 16, 1024])
def test_short_references_and_a_run_that_closes_behind_the_last_lane(ref_len):
    ref, rows = AV.small_case(ref_len, ref_len)
    want = AV.restate(rows, ref)
    with align.Aligner(ref) as al:
        for pitch in (ref_len, ref_len + 1, ref_len + 7):
            _equal(al.variants_of(AV.flat(rows, pitch), pitch), want, (ref_len, pitch))


# ------------------------------------------------------------------------------------------------------------------ through the aligner
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


def _rows_and_variants(al, got, pool, want, label):
    """the rows a call returned are the oracle's, and the records are the restatement's over those very rows"""
    score, rows = got
    w_scores, w_rows = want
    assert score.tolist() == w_scores, label
    mine = [rows[i].tobytes() for i in range(len(w_rows))]
    assert mine == w_rows, label
    _equal(al.variants(), AV.restate(mine, pool.ref), label)


@pytest.mark.parametrize("name", [p.name for p in AI.small_pools()])
def test_records_equal_the_restatement_through_every_way_in(name):
    pool = AI.pool_named(name)
    seqs = list(pool.seqs)
    scores, rows, cells, table = AI.expected(pool)
    with _aligner(pool) as al:
        al.set_variants(True)
        for ins in (False, True):
            al.set_insertions(ins)
            _rows_and_variants(al, al.align(seqs), pool, (scores, rows), (name, "align", ins))             # uvaia_align_batch
            assert al.stats()["cells"] == cells
            al.load(seqs)                                                                                    # uvaia_align_load_block / run
            al.run()
            _rows_and_variants(al, al.fetch(), pool, (scores, rows), (name, "load", ins))
            blob = np.frombuffer(b"".join(seqs) + b"\0" * 64, dtype=np.uint8).copy()                       # uvaia_align_load_device
            off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
            hip, base = _hip_runtime(), C.c_void_p()
            assert hip.hipMalloc(C.byref(base), blob.size) == 0
            try:
                assert hip.hipMemcpy(base, blob.ctypes.data, blob.size, 1) == 0
                al.load_device(base.value, off)
                al.run()
                _rows_and_variants(al, al.fetch(), pool, (scores, rows), (name, "load_device", ins))
            finally:
                hip.hipFree(base)
            if ins:
                assert al.insertions() == table, name


def test_the_long_pool_once():
    """65 700 sites: more than 64 rounds of a wave"""
    pool = AI.long_pool()
    scores, rows, cells, table = AI.expected(pool)
    with _aligner(pool) as al:
        al.set_variants(True)
        al.set_insertions(True)
        _rows_and_variants(al, al.align(list(pool.seqs)), pool, (scores, rows), "long")
        assert al.insertions() == table


# ------------------------------------------------------------------------------------------------------------------ state
def test_state_switching_and_refusals():
    pool = AI.pool_named("I-substitutions")
    seqs = list(pool.seqs)
    scores, rows, cells, table = AI.expected(pool)
    want = AV.restate(rows, pool.ref)
    names, e_rows = AV.edge_rows()
    other_ref = pool.ref
    foreign = [bytes(AE.other(other_ref[:1])) + other_ref[1:10] + b"---" + other_ref[13:], other_ref]
    want_foreign = AV.restate(foreign, other_ref)
    with _aligner(pool) as al:
        for call in (al.variants, ):
            with pytest.raises(align.AlignError) as e:                   # before any run
                call()
            assert e.value.code == ESTATE
        off = tuple(x.copy() for x in al.align(seqs))                    # off: a run leaves no answer
        st_off = al.stats()
        with pytest.raises(align.AlignError) as e:
            al.variants()
        assert e.value.code == ESTATE
        assert al.variants_ms() == 0
        al.set_variants(True)
        with pytest.raises(align.AlignError) as e:                       # on, before a run with the option on
            al.variants()
        assert e.value.code == ESTATE
        al.load(seqs)
        with pytest.raises(align.AlignError) as e:                       # on, loaded, not run
            al.variants()
        assert e.value.code == ESTATE
        al.set_insertions(True)
        al.run()
        _equal(al.variants(), want, "on")
        assert al.variants_ms(reset=True) > 0 and al.variants_ms() == 0
        # variants_of between run and fetch: rows, scores and insertions stay as they were, the answer is that of the last call
        _equal(al.variants_of(foreign), want_foreign, "variants_of between run and fetch")
        on = al.fetch()
        st_on = al.stats()
        assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and on[0].tolist() == scores
        assert al.insertions() == table
        _equal(al.variants(), want_foreign, "still the last call's")
        ptr, pitch, n, dev = al.device_rows()
        assert (pitch, n) == (len(pool.ref) + 1, len(seqs)) and ptr
        # rows, scores, cells, passes and what kernel_ms counts do not depend on the option
        assert (st_on["cells"], st_on["passes"]) == (st_off["cells"], st_off["passes"]) == (cells, 1)
        assert st_on["kernel_ms"] > 0 and st_off["kernel_ms"] > 0
        # the refusals leave the aligner usable, and the last answer in place
        L = al.L
        buf = np.frombuffer(b"".join(foreign), dtype=np.uint8).copy()
        for args in ((buf.ctypes.data, len(pool.ref) - 1, 2), (buf.ctypes.data, len(pool.ref), -1), (None, len(pool.ref), 2), (None, 0, 0)):
            assert L.uvaia_align_variants_of(al.ptr, args[0], args[1], args[2]) == EINVAL, args
            assert (L.uvaia_align_last_error(al.ptr) or b"") != b""
        _equal(al.variants(), want_foreign, "after refusals")
        assert L.uvaia_align_variants_of(al.ptr, None, len(pool.ref), 0) == 0          # n == 0 is a valid, empty answer
        rec, qc = al.variants()
        assert rec.size == 0 and qc.size == 0
        # a new load drops a run's answer but not one of variants_of; a run with the option on replaces either
        al.variants_of(foreign)
        al.load(seqs)
        _equal(al.variants(), want_foreign, "variants_of outlives a load")
        al.run()
        _equal(al.variants(), want, "the run's answer replaces it")
        al.load(seqs)
        with pytest.raises(align.AlignError) as e:
            al.variants()
        assert e.value.code == ESTATE
        # off again: the run leaves none, and nothing else changed
        al.set_variants(False)
        al.set_insertions(False)
        again = al.align(seqs)
        assert np.array_equal(again[0], off[0]) and np.array_equal(again[1], off[1])
        with pytest.raises(align.AlignError) as e:
            al.variants()
        assert e.value.code == ESTATE
        _equal(al.variants_of(foreign), want_foreign, "variants_of with the option off")
        al.align(seqs)                                                   # with the option off a run leaves variants_of's answer
        _equal(al.variants(), want_foreign, "an answer of variants_of stands over a run with the option off")
        al.set_variants(True)
        al.align([])                                                     # an empty pool: an empty answer
        rec, qc = al.variants()
        assert rec.size == 0 and qc.size == 0
        al.align(seqs[:1] + seqs)                                        # and on again
        _equal(al.variants(), AV.restate(rows[:1] + rows, pool.ref), "on again")


# ------------------------------------------------------------------------------------------------------------------ the command
ROUTES = {"text": ["-o", "{stem}"], "stdout": ["--stdout"], "packed": ["--packed", "{stem}.uvdb"], "compact": ["--packed", "{stem}.c.uvdb", "--compact"],
          "parse": ["--device-parse", "-o", "{stem}"], "devices": ["--devices", "0,0", "-o", "{stem}"], "insertions": ["-o", "{stem}", "--insertions", "{stem}.ins.csv"]}
TABLE_SUFFIX = {"text": (".var.csv.xz", ".qc.csv.gz")}


def _read(path):
    opener = lzma.open if path.endswith(".xz") else gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def commands(tmp_path_factory):
    d = tmp_path_factory.mktemp("align_variants")
    ref, names, seqs, dropped = AV.cli_case()
    (d / "ref.fa").write_bytes(b">the reference\n" + ref + b"\n")
    (d / "in.fa").write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in zip(names, seqs)))
    res = {}
    for with_tables in (False, True):                                    # seven commands at a time
        procs = {}
        for how, args in ROUTES.items():
            stem = str(d / ("%s.%s" % (how, "var" if with_tables else "plain")))
            sv, sq = TABLE_SUFFIX.get(how, (".var.csv", ".qc.csv"))
            cmd = [UVAIALIGN, "-r", str(d / "ref.fa"), "-p", "5", "-A", AI.CLI_AMBIG_R] + [a.format(stem=stem) for a in args] + (["--variants", stem + sv, "--qc", stem + sq] if with_tables else []) + [str(d / "in.fa")]
            procs[how] = (subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE), stem, (stem + sv, stem + sq))
        try:
            for how, (p, stem, tables) in procs.items():
                out, err = p.communicate(timeout=300)
                res[(how, with_tables)] = (p.returncode, out, err.decode(errors="replace"), stem, tables)
        finally:
            for p, _, _ in procs.values():
                if p.poll() is None:
                    p.kill()
                    p.communicate()
        died = [(k, r[0]) for k, r in res.items() if r[0] != 0]
        assert not died, (died, [res[k][2][-1500:] for k, _ in died[:1]])
    return d, res, AV.cli_tables(ref, names, seqs, dropped), dropped


@pytest.mark.parametrize("how", list(ROUTES))
def test_both_tables_are_the_expected_bytes_whatever_the_route(commands, how):
    d, res, (want_var, want_qc), dropped = commands
    rc, out, err, stem, (f_var, f_qc) = res[(how, True)]
    assert _read(f_var) == want_var
    assert _read(f_qc) == want_qc
    kinds = [ln.split(b",")[-5] for ln in want_var.split(b"\n")[1:-1]]
    n_seqs = want_qc.count(b"\n") - 1
    assert "Variants: %d sequences with %d substitutions, %d deletions (" % (n_seqs, kinds.count(b"S"), kinds.count(b"D")) in err, err[-1500:]
    assert ") and %d insertions (" % kinds.count(b"I") in err, err[-1500:]
    assert "Variants:" not in res[(how, False)][2]
    assert ("Insertions:" in err) == (how == "insertions")              # the insertion records are on for the tables; their own table is not written
    for p in (stem + ".ins.csv",):
        assert os.path.exists(p) == (how == "insertions")


@pytest.mark.parametrize("how", list(ROUTES))
def test_every_other_output_is_what_it_is_without_the_options(commands, how):
    d, res, want, dropped = commands
    plain, var = res[(how, False)], res[(how, True)]
    base = _read(res[("text", False)][3] + ".aln.xz")
    assert base.count(b">") == 13
    if how == "stdout":
        assert plain[1] == var[1] == base
    elif how in ("packed", "compact"):
        suffix = ".uvdb" if how == "packed" else ".c.uvdb"
        a, b = open(plain[3] + suffix, "rb").read(), open(var[3] + suffix, "rb").read()
        assert a == b and len(a) > 1024
        assert not os.path.exists(var[3] + ".aln.xz")
    else:
        assert _read(plain[3] + ".aln.xz") == _read(var[3] + ".aln.xz") == base
    if how == "insertions":
        a, b = _read(plain[3] + ".ins.csv"), _read(var[3] + ".ins.csv")
        assert a == b and a.count(b"\n") == 30
