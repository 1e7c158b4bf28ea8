"""Rows out of a packed database on a GPU box: uvaia_gpu_db_stage_unpack_rows (the text of lanes of a staging slot, decoded where the slot
lies) through the C ABI; `uvaia --packed --final-aln [--final-rank] [--final-only]` against what the command's own regular outputs say
the file must hold; membership by ordinal when two references share a name; the chunk edge of the extraction (more than 256 rows);
`uvaiapack --unpack [--names]` against the text that was packed."""
import lzma
import os
import subprocess

import numpy as np
import pytest

import compact_lib as CL
import fixtures as F
import oracle_lib as O
import packed_lib as P
from uvaia_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIA = os.path.join(ROOT, "bin", "uvaia")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")
UVAIALIGN = os.path.join(ROOT, "bin", "uvaialign")
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")
SIZES = (29, 300, 1000)
N_ROWS = 130                                                 # three tiles, the last partly filled
EINVAL, ESTATE = -1, -6                                    # UVAIA_GPU_EINVAL, UVAIA_GPU_ESTATE (include/uvaia_gpu.h)
TO_N = bytes.maketrans(P.EXCEPTIONS, b"N" * len(P.EXCEPTIONS))


def _acgt_row(nchar):
    return bytes(b"ACGT"[s & 3] for s in range(nchar))


def _queries(nchar, n=5):
    root = bytearray(_acgt_row(nchar))
    qs = []
    for i in range(n):
        s = bytearray(root)
        s[(17 * i + 3) % nchar] = ord("T") if s[(17 * i + 3) % nchar] != ord("T") else ord("A")
        qs.append(bytes(s))
    return qs, ["q%d" % i for i in range(n)]


def _rows(nchar, seed=3):
    """130 upper-case rows: awkward ones (every IUPAC code, N runs, - ? . X O, lower case in the source) and, at fixed places, all N,
    all '-', every IUPAC letter in turn, an exception run at site 0 and one at the last site"""
    rows = [s.upper() for s in P.awkward_references(N_ROWS, nchar, seed)]
    letters = b"ACGTMRWSYKVHDBN"
    run = max(1, min(7, nchar // 4))
    rows[1] = b"N" * nchar
    rows[62] = b"-" * nchar
    rows[63] = bytes(letters[s % len(letters)] for s in range(nchar))
    rows[64] = b"?" * run + _acgt_row(nchar)[run:]
    rows[129] = _acgt_row(nchar)[:nchar - run] + b"." * run
    return rows


def _tiles(tmp, rows, tag):
    """(dense tiles (planes, non_n, canonical side rows) of the rows, their compact file read back)"""
    nchar = len(rows[0])
    planes, non_n = P.pack_tiles(rows, nchar)
    side = CL.side_rows_canonical(planes, nchar)
    path = tmp / ("%s.uvdb" % tag)
    CL.write_compact(path, ["r%d" % i for i in range(len(rows))], rows, planes, non_n)
    return (planes, non_n, side), CL.CompactFile(path)


INDEX_LISTS = {"empty": [], "first": [0], "tile edge": [63, 64], "last": [129], "reversed": list(range(129, -1, -1)),
               "repeats": [5, 5, 129, 64, 5, 0, 129, 63, 63], "more than a round": [(37 * k) % 130 for k in range(300)]}


# ---------------------------------------------------------------------------------------------------------------- 1. the slot entry
@pytest.mark.parametrize("acgt", [False, True])
@pytest.mark.parametrize("nchar", SIZES)
def test_rows_of_a_staged_slot(tmp_path, nchar, acgt):
    rows = _rows(nchar)
    want = [r.translate(TO_N) for r in rows]
    dense, cf = _tiles(tmp_path, rows, "all")
    dense_a, _ = _tiles(tmp_path, rows[:70], "a")                                  # two files for the slot of two pieces: 70 rows, then 60
    _, cf_b = _tiles(tmp_path, rows[70:], "b")
    qs, qn = _queries(nchar)
    with capi.Engine.from_query(O.Query(qs, qn, acgt=acgt), nbest=2, max_pool=64) as eng:   # a pool of 64: 300 indices are five rounds
        eng.db_stage_reserve(3)
        for how in ("dense", "compact", "two pieces"):
            slot = 1 if how == "compact" else 0
            # the slot holds other bytes before: all ones in every plane
            eng.db_stage_packed(slot, np.full_like(dense[0], 0xFF), np.full_like(dense[1], -1), np.full_like(dense[2], -1), 3)
            pos = lambda i: i
            if how == "dense":
                eng.db_stage_packed(slot, *dense, 3)
            elif how == "compact":
                eng.db_stage_compact_at(slot, 0, *cf.stage_args(0, 3))
            else:
                eng.db_stage_packed_at(slot, 0, *dense_a, 2)
                eng.db_stage_compact_at(slot, 2, *cf_b.stage_args(0, 1))
                pos = lambda i: i if i < 70 else 128 + (i - 70)                    # the second file starts at tile 2 of the slot
            for what, index in INDEX_LISTS.items():
                got = eng.db_stage_unpack_rows(slot, [pos(i) for i in index])
                assert got == [want[i] for i in index], (how, what)
            # a pitch that is not the staging pitch: the strided copy back
            assert eng.db_stage_unpack_rows(slot, [pos(129), pos(0)], pitch=nchar + 3) == [want[129], want[0]], how
        assert eng.stage_unpack_ms() > 0.
        assert eng.stage_unpack_ms(reset=True) > 0. and eng.stage_unpack_ms() == 0.
        assert eng.db_size() == 0                                                  # nothing became resident on the way


@pytest.mark.parametrize("acgt", [False, True])
def test_the_call_leaves_database_window_and_heaps_alone(tmp_path, acgt):
    nchar, n, nq = 300, 200, 40                                                    # 40 queries: the scan that keeps planes derived for the query set
    seqs = CL.near_identical_references(n + nq, nchar, 11)
    refs, qs = [s.upper() for s in seqs[:n]], [s.replace(b"N", b"A").replace(b"-", b"C") for s in seqs[n:]]
    planes, non_n = P.pack_tiles(refs, nchar)
    resident = (planes, non_n, CL.side_rows_canonical(planes, nchar))
    rows = _rows(nchar)
    dense, _ = _tiles(tmp_path, rows, "other")
    with capi.Engine.from_query(O.Query(qs, ["q%d" % i for i in range(nq)], acgt=acgt), nbest=4, max_pool=64) as eng:
        eng.db_reserve(256)
        eng.db_stage_reserve(4)
        eng.db_stage_packed(0, *resident, 4)
        eng.db_load_staged(0, None, n)                                             # a loaded window, so db_unpack_rows has its image
        ent = eng.search_resident(64)
        assert ent.any()
        # (the interchange form is exported from a default-mode context only; the text of every resident row and the derived planes
        # stand for the database in both)
        state = lambda: (list(() if acgt else eng.db_export()) + list(eng.db_derived(4)), eng.drain(), eng.db_unpack_rows(list(range(n))), eng.db_size())
        before = state()
        eng.db_stage_packed(1, *dense, 3)
        got = eng.db_stage_unpack_rows(1, list(range(N_ROWS)))
        assert got == [r.translate(TO_N) for r in rows]
        after = state()
        for x, y in zip(list(before[0]) + list(before[1]), list(after[0]) + list(after[1])):
            assert np.array_equal(x, y)
        assert before[2:] == after[2:]
        # and a search after it is the search of a context that never made the call (the heaps drained above)
        eng.reset()
        assert np.array_equal(eng.search_resident(64), ent)
        for x, y in zip(eng.drain(), before[1]):
            assert np.array_equal(x, y)


def test_refusals_leave_the_context_usable(tmp_path):
    nchar = 300
    rows = _rows(nchar)
    want = [r.translate(TO_N) for r in rows]
    dense, _ = _tiles(tmp_path, rows, "r")
    qs, qn = _queries(nchar)
    with capi.Engine.from_query(O.Query(qs, qn), nbest=2, max_pool=64) as eng:
        with pytest.raises(capi.GpuError) as ei:                                   # never staged, not even reserved
            eng.db_stage_unpack_rows(0, [0])
        assert ei.value.code == ESTATE
        eng.db_stage_reserve(3)
        eng.db_stage_packed(0, *dense, 3)
        assert eng.db_stage_unpack_rows(0, [129]) == [want[129]]
        for slot, index, pitch, code in ((0, [0, 192], None, EINVAL), (0, [-1], None, EINVAL), (1, [0], None, ESTATE), (1, [], None, ESTATE), (0, [0], nchar - 1, EINVAL), (2, [0], None, EINVAL)):
            with pytest.raises(capi.GpuError) as ei:
                eng.db_stage_unpack_rows(slot, index, pitch=pitch)
            assert ei.value.code == code, (slot, index, pitch)
            assert eng.db_stage_unpack_rows(0, [191, 0]) == [b"N" * nchar, want[0]]  # lane 191: a zero lane past the last reference
        # a slot that was cut down to two tiles by a new first piece
        eng.db_stage_packed(0, *dense, 2)
        with pytest.raises(capi.GpuError):
            eng.db_stage_unpack_rows(0, [128])
        assert eng.db_stage_unpack_rows(0, [127]) == [want[127]]


# ---------------------------------------------------------------------------------------------------------------- command lines
def _write_fasta(path, names, seqs, opener=open):
    with opener(path, "wb") as fh:
        for n, s in zip(names, seqs):
            fh.write(b">" + n.encode() + b"\n" + s + b"\n")


def _run(cmd, ok=True, stdout=subprocess.DEVNULL):
    r = subprocess.run(cmd, stdout=stdout, stderr=subprocess.PIPE, timeout=600)
    assert (r.returncode == 0) == ok, (cmd, r.stderr[-2000:])
    return r.stderr.decode(errors="replace") if stdout is subprocess.DEVNULL else (r.stdout, r.stderr.decode(errors="replace"))


def _run_together(cmds, stdout=False):
    """independent commands, at most ten at once (each opens the GPU for a moment): their stderr texts, with stdout=True (stdout, stderr) pairs"""
    logs = []
    for a in range(0, len(cmds), 10):
        procs = [subprocess.Popen(c, stdout=subprocess.PIPE if stdout else subprocess.DEVNULL, stderr=subprocess.PIPE) for c in cmds[a:a + 10]]
        for c, p in zip(cmds[a:], procs):
            out, err = p.communicate(timeout=600)
            assert p.returncode == 0, (c, err[-2000:])
            logs.append((out, err.decode(errors="replace")) if stdout else err.decode(errors="replace"))
    return logs


def _xz(prefix, suffix):
    return lzma.open(prefix + suffix, "rb").read()


def _records(data):
    """[(header line, sequence line)] of a FASTA the commands wrote: two lines per record"""
    lines = data.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    recs = list(zip(lines[0:-1:2], lines[1:-1:2]))
    assert all(h.startswith(b">") for h, _ in recs)
    return recs


def _expected_final(prefix, rank):
    """the records of the regular dump whose name is in column 2 of the table with rank <= `rank`, in file order: nothing of it comes
    from the code under test.  Also the number of distinct names."""
    names = set()
    for line in _xz(prefix, ".csv.xz").split(b"\n")[1:]:
        if line:
            cols = line.split(b",")
            if int(cols[2]) <= rank:
                names.add(cols[1])
    recs = [r for r in _records(_xz(prefix, ".aln.xz")) if r[0][1:] in names]
    assert len(recs) == len(names)                                                 # unique names: one record each
    return b"".join(h + b"\n" + s + b"\n" for h, s in recs), len(names)


NCOL = 1000
N_A, N_B = 230, 100                                          # a cut of the bundled alignment; an awkward set (both end inside a tile)
NBEST = 4


@pytest.fixture(scope="module")
def cli(tmp_path_factory, bundled_db):
    """the command-line fixture of test_uvdb_compact_gpu.py"""
    d = tmp_path_factory.mktemp("extract_cli")
    names, seqs = bundled_db
    cols = np.linspace(400, 29400, NCOL).astype(np.int64)
    pick = lambda s: np.frombuffer(s, dtype=np.uint8)[cols].tobytes().upper()
    a, an = [pick(s) for s in seqs[:N_A]], list(names[:N_A])
    b, bn = [s.upper() for s in P.awkward_references(N_B, NCOL, 5)], ["awk%d" % i for i in range(N_B)]
    assert len(set(an + bn)) == N_A + N_B
    _write_fasta(d / "a.fa", an, a)
    _write_fasta(d / "b.fa", bn, b)
    f = {k: str(d / k) for k in ("a.fa", "b.fa", "q.fa", "dense.uvdb", "compact.uvdb", "dense_a.uvdb", "compact_b.uvdb")}
    _run_together([[UVAIAPACK, "-A", "0.9", "-o", f["dense.uvdb"], f["a.fa"], f["b.fa"]],
                   [UVAIAPACK, "-A", "0.9", "--compact", "-o", f["compact.uvdb"], f["a.fa"], f["b.fa"]],
                   [UVAIAPACK, "-A", "0.9", "-o", f["dense_a.uvdb"], f["a.fa"]],
                   [UVAIAPACK, "-A", "0.9", "--compact", "-o", f["compact_b.uvdb"], f["b.fa"]]])
    assert CL.file_version(f["compact.uvdb"]) == 2 and CL.file_version(f["dense.uvdb"]) == 1
    qs = [pick(s) for s in seqs[1000:1006]]
    qn = [an[70], bn[3]] + ["query%d" % i for i in range(4)]                  # two of them named like references: -x drops those
    _write_fasta(d / "q.fa", qn, qs)
    return d, f


# ---------------------------------------------------------------------------------------------------------------- 2. --final-aln
@pytest.mark.parametrize("db", ["dense", "compact", "set"])
@pytest.mark.parametrize("acgt", [[], ["--acgt"]])
@pytest.mark.parametrize("exclude", [[], ["-x"]])
@pytest.mark.parametrize("window", [[], ["--window", "96"]])
def test_final_alignment_is_the_filter_of_the_regular_outputs(cli, window, exclude, acgt, db):
    d, f = cli
    tag = db + "".join(x.strip("-") for x in window + exclude + acgt)
    packed = {"dense": ["--packed", f["dense.uvdb"]], "compact": ["--packed", f["compact.uvdb"]], "set": ["--packed", f["dense_a.uvdb"], "--packed", f["compact_b.uvdb"]]}[db]
    base = [UVAIA, f["q.fa"], "-n", str(NBEST), "-A", "0.9", "-p", "64"] + window + exclude + acgt + packed
    out = lambda k: str(d / ("%s_%s" % (tag, k)))
    runs = {"plain": [], "final": ["--final-aln"], "r1": ["--final-aln", "--final-rank", "1"], "r2": ["--final-aln", "--final-rank", "2"],
            "r9": ["--final-aln", "--final-rank", "9"], "only": ["--final-aln", "--final-only"], "only2": ["--final-aln", "--final-rank", "2", "--final-only"]}
    logs = dict(zip(runs, _run_together([base + extra + ["-o", out(k)] for k, extra in runs.items()])))
    table, dump = _xz(out("plain"), ".csv.xz"), _xz(out("plain"), ".aln.xz")
    assert len(table) > 500 and len(dump) > 5 * NCOL
    assert not os.path.exists(out("plain") + ".final.aln.xz")
    want = {r: _expected_final(out("plain"), r) for r in (1, 2, NBEST)}
    assert 0 < want[1][1] < want[2][1] < want[NBEST][1] < len(_records(dump))      # the ranks differ, and the dump holds more than the final lists
    for k, rank in (("final", NBEST), ("r1", 1), ("r2", 2), ("r9", NBEST), ("only", NBEST), ("only2", 2)):
        assert _xz(out(k), ".csv.xz") == table, k
        assert _xz(out(k), ".final.aln.xz") == want[rank][0], k
        assert "Saved %d sequences of the final neighbour lists" % want[rank][1] in logs[k], k
        if k.startswith("only"):
            assert not os.path.exists(out(k) + ".aln.xz"), k
        else:
            assert _xz(out(k), ".aln.xz") == dump, k


def test_final_alignment_follows_the_acgt_prefix_rule(cli, tmp_path):
    d, f = cli
    r = subprocess.run([UVAIA, f["q.fa"], "-n", str(NBEST), "-A", "0.9", "-p", "64", "--acgt", "--final-aln", "--packed", f["dense.uvdb"]],
                       cwd=str(tmp_path), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(str(tmp_path))) == ["nn_uvaia_acgt.aln.xz", "nn_uvaia_acgt.csv.xz", "nn_uvaia_acgt.final.aln.xz"]
    assert _xz(str(tmp_path / "nn_uvaia_acgt"), ".final.aln.xz") == _expected_final(str(tmp_path / "nn_uvaia_acgt"), NBEST)[0]


# ---------------------------------------------------------------------------------------------------------------- 3. by ordinal
@pytest.mark.parametrize("window", [[], ["--window", "64"]])
@pytest.mark.parametrize("two_files", [False, True])
def test_membership_is_by_ordinal_not_by_name(tmp_path, two_files, window):
    nchar = 200
    close = _acgt_row(nchar)
    rng = np.random.default_rng(17)
    far = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nchar))    # a random row: about a quarter of the sites match
    filler = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nchar)) for _ in range(98)]
    seqs = [far] + filler[:69] + [close] + filler[69:]                             # the far one first, the close one at 70: the second tile
    names = ["twin"] + ["f%d" % i for i in range(69)] + ["twin"] + ["f%d" % i for i in range(69, 98)]
    _write_fasta(tmp_path / "q.fa", ["the query"], [close])
    if two_files:
        _write_fasta(tmp_path / "a.fa", names[:40], seqs[:40])
        _write_fasta(tmp_path / "b.fa", names[40:], seqs[40:])
        _run_together([[UVAIAPACK, "-o", str(tmp_path / "a.uvdb"), str(tmp_path / "a.fa")], [UVAIAPACK, "--compact", "-o", str(tmp_path / "b.uvdb"), str(tmp_path / "b.fa")]])
        packed = ["--packed", str(tmp_path / "a.uvdb"), "--packed", str(tmp_path / "b.uvdb")]
    else:
        _write_fasta(tmp_path / "a.fa", names, seqs)
        _run([UVAIAPACK, "-o", str(tmp_path / "a.uvdb"), str(tmp_path / "a.fa")])
        packed = ["--packed", str(tmp_path / "a.uvdb")]
    prefix = str(tmp_path / "out")
    _run([UVAIA, str(tmp_path / "q.fa"), "-n", "1", "-p", "64", "--final-aln", "-o", prefix] + window + packed)
    dump = _records(_xz(prefix, ".aln.xz"))
    assert (b">twin", far) in dump and (b">twin", close) in dump                   # the far one entered the empty heap: it is in the regular dump
    rows = [l.split(b",") for l in _xz(prefix, ".csv.xz").split(b"\n")[1:] if l]
    assert [r[1] for r in rows if int(r[2]) == 1] == [b"twin"] and int([r for r in rows if int(r[2]) == 1][0][3]) == nchar
    assert _xz(prefix, ".final.aln.xz") == b">twin\n" + close + b"\n"              # one record, the close one's sequence


# ---------------------------------------------------------------------------------------------------------------- 4. the chunk edge
@pytest.mark.parametrize("window", [[], ["--window", "192"]])
def test_more_final_members_than_one_chunk(tmp_path_factory, window):
    """600 references at 500 sites, 70 queries that are copies of different references with two substitutions, -n 8: more than 256
    distinct references are in the table, i.e. more than one chunk of the extraction (generator seed 2024; the count is asserted below on the
    table of the run without the option, which the search of the parent commit writes byte for byte)."""
    d = tmp_path_factory.mktemp("chunk_edge")
    nchar, n, nq = 500, 600, 70
    rng = np.random.default_rng(2024)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    refs = [bytes(rng.choice(acgt, size=nchar)) for _ in range(n)]
    qs = []
    for k in range(nq):
        s = bytearray(refs[(k * 8 + 3) % n])
        for site in (7 + k, 300 + 2 * k):
            s[site] = ord("A") if s[site] != ord("A") else ord("C")
        qs.append(bytes(s))
    _write_fasta(d / "r.fa", ["ref%d" % i for i in range(n)], refs)
    _write_fasta(d / "q.fa", ["query%d" % k for k in range(nq)], qs)
    _run([UVAIAPACK, "--compact", "-o", str(d / "r.uvdb"), str(d / "r.fa")])
    base = [UVAIA, str(d / "q.fa"), "-n", "8", "-p", "64", "--packed", str(d / "r.uvdb")] + window
    _run_together([base + ["-o", str(d / "plain")], base + ["--final-aln", "-o", str(d / "final")], base + ["--final-aln", "--final-only", "-o", str(d / "only")]])
    want, n_final = _expected_final(str(d / "plain"), 8)
    print("distinct references in the table: %d" % n_final)
    assert n_final >= 257
    for k in ("final", "only"):
        assert _xz(str(d / k), ".csv.xz") == _xz(str(d / "plain"), ".csv.xz")
        assert _xz(str(d / k), ".final.aln.xz") == want, k
    assert _xz(str(d / "final"), ".aln.xz") == _xz(str(d / "plain"), ".aln.xz")


# ---------------------------------------------------------------------------------------------------------------- 5. small ends
def test_a_database_of_one_reference(tmp_path):
    row = _acgt_row(131)[:100] + b"-" * 20 + b"RYKMSWBDHVN"
    _write_fasta(tmp_path / "r.fa", ["the only one"], [row])
    _write_fasta(tmp_path / "q.fa", ["q"], [_acgt_row(131)])
    _run([UVAIAPACK, "-o", str(tmp_path / "r.uvdb"), str(tmp_path / "r.fa")])
    for extra, prefix in (([], "p"), (["--final-only"], "o"), (["--window", "64"], "w")):
        _run([UVAIA, str(tmp_path / "q.fa"), "-n", "3", "--final-aln", "--packed", str(tmp_path / "r.uvdb"), "-o", str(tmp_path / prefix)] + extra)
        assert _xz(str(tmp_path / prefix), ".final.aln.xz") == b">the only one\n" + row + b"\n"
    assert _xz(str(tmp_path / "p"), ".aln.xz") == _xz(str(tmp_path / "p"), ".final.aln.xz")
    assert _xz(str(tmp_path / "o"), ".csv.xz") == _xz(str(tmp_path / "p"), ".csv.xz")


def test_heaps_that_are_not_full(tmp_path):
    nchar = 300
    refs = [s.upper() for s in CL.near_identical_references(40, nchar, 5)]
    _write_fasta(tmp_path / "r.fa", ["ref%d" % i for i in range(40)], refs)
    _write_fasta(tmp_path / "q.fa", ["q0", "q1"], [refs[3].replace(b"N", b"A").replace(b"-", b"C"), refs[30].replace(b"N", b"A").replace(b"-", b"C")])
    _run([UVAIAPACK, "-A", "0.9", "-o", str(tmp_path / "r.uvdb"), str(tmp_path / "r.fa")])
    base = [UVAIA, str(tmp_path / "q.fa"), "-n", "100", "-A", "0.9", "-p", "64", "--packed", str(tmp_path / "r.uvdb")]
    _run_together([base + ["-o", str(tmp_path / "plain")], base + ["--final-aln", "-o", str(tmp_path / "final")], base + ["--final-aln", "--final-rank", "3", "-o", str(tmp_path / "r3")]])
    want, n_final = _expected_final(str(tmp_path / "plain"), 100)
    assert n_final == len(_records(_xz(str(tmp_path / "plain"), ".aln.xz"))) >= 30  # the heaps are not full: whatever entered one is still in it
    assert _xz(str(tmp_path / "final"), ".final.aln.xz") == want == _xz(str(tmp_path / "plain"), ".aln.xz")
    assert _xz(str(tmp_path / "r3"), ".final.aln.xz") == _expected_final(str(tmp_path / "plain"), 3)[0]


@pytest.mark.parametrize("window", [[], ["--window", "64"]])
def test_a_member_in_the_partly_filled_last_tile_of_the_first_file(tmp_path, window):
    nchar = 300
    seqs = [s.upper() for s in CL.near_identical_references(110, nchar, 9)]
    rng = np.random.default_rng(4)
    far = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nchar)) for _ in range(110)]
    refs = [far[i] if i != 69 else seqs[i] for i in range(110)]                    # only reference 69 is near the query
    names = ["ref%d" % i for i in range(110)]
    _write_fasta(tmp_path / "a.fa", names[:70], refs[:70])                          # 70 references: lane 5 of the second tile is the file's last
    _write_fasta(tmp_path / "b.fa", names[70:], refs[70:])
    _write_fasta(tmp_path / "q.fa", ["q"], [seqs[69].replace(b"N", b"A").replace(b"-", b"C")])
    _run_together([[UVAIAPACK, "-A", "0.9", "--compact", "-o", str(tmp_path / "a.uvdb"), str(tmp_path / "a.fa")], [UVAIAPACK, "-A", "0.9", "-o", str(tmp_path / "b.uvdb"), str(tmp_path / "b.fa")]])
    base = [UVAIA, str(tmp_path / "q.fa"), "-n", "2", "-A", "0.9", "-p", "64", "--packed", str(tmp_path / "a.uvdb"), "--packed", str(tmp_path / "b.uvdb")] + window
    _run_together([base + ["-o", str(tmp_path / "plain")], base + ["--final-aln", "--final-rank", "1", "-o", str(tmp_path / "final")]])
    assert _xz(str(tmp_path / "final"), ".final.aln.xz") == b">ref69\n" + refs[69] + b"\n" == _expected_final(str(tmp_path / "plain"), 1)[0]


# ---------------------------------------------------------------------------------------------------------------- 6. uvaiapack --unpack
def _fasta(names, rows):
    return b"".join(b">" + n.encode() + b"\n" + r + b"\n" for n, r in zip(names, rows))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("nchar", SIZES)
def test_unpack_gives_back_what_was_packed(tmp_path, nchar, n):
    """-A 0.999 keeps every row at 29 and 300 sites; at 1 000 sites its threshold is one valid site, which the all-N and the all-gap row
    miss, so -A 1 is used there: the point of the value is that no row is dropped."""
    rows, names = _rows(nchar)[:n], ["seq %d|x" % i for i in range(n)]
    ambig = "0.999" if nchar < 1000 else "1"
    _write_fasta(tmp_path / "in.fa", names, rows)
    files = {"dense": [str(tmp_path / "d.uvdb")], "compact": [str(tmp_path / "c.uvdb")]}
    packs = [[UVAIAPACK, "-A", ambig, "-o", files["dense"][0], str(tmp_path / "in.fa")], [UVAIAPACK, "-A", ambig, "--compact", "-o", files["compact"][0], str(tmp_path / "in.fa")]]
    if n > 1:                                                                      # two files of different form: the first ends inside a tile
        cut = n // 2 + 1
        _write_fasta(tmp_path / "lo.fa", names[:cut], rows[:cut])
        _write_fasta(tmp_path / "hi.fa", names[cut:], rows[cut:])
        files["two"] = [str(tmp_path / "lo.uvdb"), str(tmp_path / "hi.uvdb")]
        packs += [[UVAIAPACK, "-A", ambig, "--compact", "-o", files["two"][0], str(tmp_path / "lo.fa")], [UVAIAPACK, "-A", ambig, "-o", files["two"][1], str(tmp_path / "hi.fa")]]
    _run_together(packs)
    cases = [(how, paths, str(tmp_path / ("u_" + how))) for how, paths in files.items()]
    got = _run_together([[UVAIAPACK, "--unpack", "-o", prefix] + paths for _, paths, prefix in cases] + [[UVAIAPACK, "--unpack", "--stdout"] + paths for _, paths, _ in cases], stdout=True)
    want = _fasta(names, rows)
    for k, (how, _, prefix) in enumerate(cases):
        assert _xz(prefix, ".aln.xz") == want, how
        assert "Unpacked %d of %d sequences" % (n, n) in got[k][1], how
        assert got[len(cases) + k][0] == want, how


def test_unpack_by_names(tmp_path):
    nchar = 300
    rows = _rows(nchar)
    names = ["seq%d" % i for i in range(N_ROWS)]
    names[7] = names[100] = "carried twice"                                        # in two tiles
    _write_fasta(tmp_path / "lo.fa", names[:70], rows[:70])
    _write_fasta(tmp_path / "hi.fa", names[70:], rows[70:])
    _run_together([[UVAIAPACK, "-A", "0.999", "-o", str(tmp_path / "lo.uvdb"), str(tmp_path / "lo.fa")],
                   [UVAIAPACK, "-A", "0.999", "--compact", "-o", str(tmp_path / "hi.uvdb"), str(tmp_path / "hi.fa")]])
    (tmp_path / "names.txt").write_bytes(b"seq129\nnobody of that name\ncarried twice\nseq0\n\nseq129\n")
    out, log = _run([UVAIAPACK, "--unpack", "--stdout", "--names", str(tmp_path / "names.txt"), str(tmp_path / "lo.uvdb"), str(tmp_path / "hi.uvdb")], stdout=subprocess.PIPE)
    picked = [0, 7, 100, 129]
    assert out == _fasta([names[i] for i in picked], [rows[i] for i in picked])
    assert "1 of the 4 names" in log and "\n  nobody of that name\n" in log
    assert "seq129\n" not in log.split("match no reference:")[1]
    # nothing matches: an empty alignment, every name listed, still exit status 0
    (tmp_path / "none.txt").write_bytes(b"x\ny\n")
    prefix = str(tmp_path / "none")
    log = _run([UVAIAPACK, "--unpack", "-o", prefix, "--names", str(tmp_path / "none.txt"), str(tmp_path / "lo.uvdb")])
    assert _xz(prefix, ".aln.xz") == b"" and "2 of the 2 names" in log


def test_unpack_of_what_uvaialign_and_uvaiaclust_packed(tmp_path, bundled_db):
    # uvaialign --packed: the aligned rows, never text on the host
    ref = F.random_acgt(700, 31)
    seqs = F.unaligned_queries(ref, 90, 32, p_indel=0.0015, n_runs=(10, 10, 40))
    _write_fasta(tmp_path / "ref.fa", ["the reference"], [ref])
    _write_fasta(tmp_path / "raw.fa", ["hCoV-19/seq %d|2021" % i for i in range(len(seqs))], seqs)
    common = [UVAIALIGN, "-r", str(tmp_path / "ref.fa"), str(tmp_path / "raw.fa"), "-p", "64"]
    # uvaiaclust --packed-out: the medoids it keeps
    names, rows = bundled_db
    cols = np.linspace(400, 29400, NCOL).astype(np.int64)
    _write_fasta(tmp_path / "in.fa", names[:300], [np.frombuffer(s, dtype=np.uint8)[cols].tobytes() for s in rows[:300]])
    _run_together([common + ["-o", str(tmp_path / "t")], common + ["--packed", str(tmp_path / "a.uvdb"), "-A", "1", "--compact"],
                   [UVAIACLUST, "-d", "4", "-s", "2", "-p", "64", "--packed-out", str(tmp_path / "c.uvdb"), "-o", str(tmp_path / "clust"), str(tmp_path / "in.fa")]])
    for db, text in (("a.uvdb", "t"), ("c.uvdb", "clust")):
        out, _ = _run([UVAIAPACK, "--unpack", "--stdout", str(tmp_path / db)], stdout=subprocess.PIPE)
        want = _xz(str(tmp_path / text), ".aln.xz")
        assert len(_records(want)) > 64 and out == want, db
