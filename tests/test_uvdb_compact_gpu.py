"""The compact form of a packed database on a GPU box: uvaia_gpu_db_stage_compact_at (expand_tiles_kernel and the side-row pass behind it)
against the dense staging of the same references, in pieces, in an --acgt context and window after window; and the command lines:
`uvaiapack --compact`, `uvaia --packed` on compact files, both directions of `uvaiapack --merge`, the three refusals."""
import lzma
import os
import subprocess

import numpy as np
import pytest

import compact_lib as CL
import oracle_lib as O
import packed_lib as P
from uvaia_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIA = os.path.join(ROOT, "bin", "uvaia")
UVAIABALL = os.path.join(ROOT, "bin", "uvaiaball")
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")
WHAT = ("planes", "non_n", "side rows")


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


def _files(tmp, seqs, tag):
    """(dense tiles (planes, non_n, canonical side rows) of the references, their compact file read back, upper-case text)"""
    up = [s.upper() for s in seqs]
    nchar = len(up[0])
    planes, non_n = P.pack_tiles(up, nchar)
    side = CL.side_rows_canonical(planes, nchar)
    path = tmp / ("%s.uvdb" % tag)
    CL.write_compact(path, ["r%d" % i for i in range(len(up))], up, planes, non_n)
    return (planes, non_n, side), CL.CompactFile(path), up


def _mixed(n, nchar, seed):
    """awkward references (every IUPAC code, side rows that are cut) among near-identical ones"""
    a, b = P.awkward_references(n, nchar, seed), CL.near_identical_references(n, nchar, seed + 1)
    return [a[i] if i % 3 == 0 else b[i] for i in range(n)]


def _assert_same(got, want, note):
    for g, w, what in zip(got, want, WHAT):
        assert np.array_equal(g, w), (note, what)


# ---------------------------------------------------------------------------------------------------------------- kernel against host expansion
@pytest.mark.parametrize("nchar", [29, 130, 1000])
def test_compact_staging_is_the_dense_staging(tmp_path, nchar):
    qs, qn = _queries(nchar)
    with capi.Engine.from_query(O.Query(qs, qn), nbest=2, max_pool=64) as eng:
        eng.db_reserve(192)
        eng.db_stage_reserve(3)
        for n_ref in (1, 63, 64, 65, 130):
            dense, cf, _ = _files(tmp_path, _mixed(n_ref, nchar, 100 + n_ref), "c%d" % n_ref)
            nt = dense[0].shape[0]
            eng.db_clear()
            eng.db_stage_packed(0, *dense, nt)
            eng.db_append_staged(0, None, n_ref)
            want = eng.db_export()
            # the slot holds other bytes before: all ones in every plane, count and side row
            eng.db_stage_packed(1, np.full_like(dense[0], 0xFF), np.full_like(dense[1], -1), np.full_like(dense[2], -1), nt)
            eng.db_clear()
            eng.db_stage_compact_at(1, 0, *cf.stage_args(0, nt))
            eng.db_append_staged(1, None, n_ref)
            _assert_same(eng.db_export(), want, (nchar, n_ref))
            assert np.array_equal(eng.db_export()[0], dense[0])                   # and the host's own tiles
            # every staged lane, those past the last reference included: zeros there, as the dense file holds them
            eng.db_clear()
            eng.db_append_staged(1, None, nt * 64)
            _assert_same(eng.db_export(), dense, (nchar, n_ref, "all lanes"))
            if n_ref % 64:
                got = eng.db_export()
                assert not got[0].reshape(nt, -1, 64, 16)[-1, :, n_ref % 64:, :].any() and not got[1][n_ref:].any() and not got[2][n_ref:].any()


def _with_heads(base, k, all_literal=False):
    """the base row with k heads: word w < k differs, even words by one site (a literal), odd words as a run of N (a fill)"""
    s = bytearray(base)
    for w in range(k):
        if all_literal or w % 2 == 0:
            s[32 * w + 5] = ord("R")
        else:
            s[32 * w:32 * w + 32] = b"N" * 32
    return bytes(s)


def test_head_count_edges(tmp_path):
    """0, 64, 65 and 130 heads in one reference -- the rounds of 64 heads and the carry of the literal prefix sum -- in lanes 0, 3, 4 and 63
    (lanes 3 and 4 fall to different waves), a reference whose every word is a literal, one fill of all words next to a lane without
    heads.  130 heads need 130 words: 4200 sites (1000 sites are 32 words only)."""
    nchar = 4200
    base = _acgt_row(nchar)
    n_real = (nchar + 31) // 32                                                    # 132 words, the last one of 8 sites
    every = _with_heads(base, n_real, all_literal=True)
    tile0 = {0: _with_heads(base, 130), 3: _with_heads(base, 64), 4: _with_heads(base, 65), 63: every, 10: b"N" * nchar}
    tile1 = {0: _with_heads(base, 64), 3: _with_heads(base, 130), 4: b"N" * nchar, 62: _with_heads(base, 65), 63: _with_heads(base, 130)}
    seqs = [tile0.get(i, base) for i in range(64)] + [tile1.get(i, base) for i in range(64)]
    dense, cf, _ = _files(tmp_path, seqs, "heads")
    count = lambda i: int(cf.head_idx[i + 1] - cf.head_idx[i])
    assert [count(i) for i in (0, 3, 4, 63, 10, 11)] == [130, 64, 65, 1, 1, 0]
    assert cf.heads_of(63) == [(0, n_real, 1, 0)] and cf.heads_of(10) == [(0, n_real, 0, 0)]      # every word a literal; one fill of all words
    assert [count(64 + i) for i in (0, 3, 4, 5, 62, 63)] == [64, 130, 1, 0, 65, 130]
    assert int(cf.lit_idx[1] - cf.lit_idx[0]) == 65 and int(cf.lit_idx[64] - cf.lit_idx[63]) == n_real
    qs, qn = _queries(nchar)
    with capi.Engine.from_query(O.Query(qs, qn), nbest=2, max_pool=64) as eng:
        eng.db_reserve(128)
        eng.db_stage_reserve(2)
        eng.db_stage_compact_at(0, 0, *cf.stage_args(0, 2))
        eng.db_append_staged(0, None, 128)
        _assert_same(eng.db_export(), dense, "head counts")
        # tile 1 alone: the index entries of a range that does not start the file
        eng.db_clear()
        eng.db_stage_compact_at(1, 0, *cf.stage_args(1, 1))
        eng.db_append_staged(1, None, 64)
        _assert_same(eng.db_export(), (dense[0][1:], dense[1][64:], dense[2][64:]), "second tile")


# ---------------------------------------------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("n_first", [5, 63])
def test_pieces_of_two_files_in_one_slot(tmp_path, n_first):
    nchar, n_second = 130, 70
    qs, qn = _queries(nchar)
    dense_a, cf_a, _ = _files(tmp_path, _mixed(n_first, nchar, 7), "a")
    dense_b, cf_b, _ = _files(tmp_path, _mixed(n_second, nchar, 8), "b")
    sel = list(range(n_first)) + [64 + i for i in range(n_second)]
    drop = {sel[0], sel[-1], sel[len(sel) // 2]}                                   # the first, the last and a middle lane
    sel = [s for s in sel if s not in drop]
    with capi.Engine.from_query(O.Query(qs, qn), nbest=2, max_pool=64) as eng:
        eng.db_reserve(192)
        eng.db_stage_reserve(3)
        eng.db_stage_packed_at(0, 0, *dense_a, 1)
        eng.db_stage_packed_at(0, 1, *dense_b, 2)
        eng.db_append_staged(0, sel, len(sel))
        want = eng.db_export()
        eng.db_clear()
        eng.db_stage_compact_at(1, 0, *cf_a.stage_args(0, 1))
        eng.db_stage_compact_at(1, 1, *cf_b.stage_args(0, 2))
        eng.db_append_staged(1, sel, len(sel))
        _assert_same(eng.db_export(), want, n_first)
        # a dense piece and a compact piece in one slot
        eng.db_clear()
        eng.db_stage_packed_at(0, 0, *dense_a, 1)
        eng.db_stage_compact_at(0, 1, *cf_b.stage_args(0, 2))
        eng.db_append_staged(0, sel, len(sel))
        _assert_same(eng.db_export(), want, (n_first, "mixed"))
        with pytest.raises(capi.GpuError):                                         # beyond the reserved capacity, as the dense call
            eng.db_stage_compact_at(0, 2, *cf_b.stage_args(0, 2))


# ---------------------------------------------------------------------------------------------------------------- --acgt context, windows
def _search_set(n, nchar, seed):
    seqs = CL.near_identical_references(n + 5, nchar, seed)
    qs = [s.replace(b"N", b"A").replace(b"-", b"C") for s in seqs[n:]]
    return seqs[:n], qs, ["q%d" % i for i in range(5)]


def test_acgt_context(tmp_path):
    nchar, n = 331, 150
    refs, qs, qn = _search_set(n, nchar, 21)
    refs = [r if i % 4 else a for i, (r, a) in enumerate(zip(refs, P.awkward_references(n, nchar, 22)))]
    dense, cf, up = _files(tmp_path, refs, "acgt")
    index = [0, 1, 63, 64, 100, n - 1]
    with capi.Engine.from_query(O.Query(qs, qn, acgt=True), nbest=4, max_pool=64) as eng:
        eng.db_reserve(n)
        eng.db_stage_reserve(3)
        eng.db_stage_packed(0, *dense, 3)
        eng.db_load_staged(0, None, n)
        ent = eng.search_resident(64)
        want, want_rows = eng.drain(), eng.db_unpack_rows(index)
        eng.reset()
        eng.db_stage_compact_at(1, 0, *cf.stage_args(0, 3))
        eng.db_load_staged(1, None, n)
        got_ent = eng.search_resident(64)
        got, got_rows = eng.drain(), eng.db_unpack_rows(index)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)) and np.array_equal(got_ent, ent)
        assert got_rows == want_rows
        assert ent.any()


@pytest.mark.parametrize("nq", [5, 40])
def test_windows_from_compact_slots(tmp_path, nq):
    """load_staged from compact-staged slots, window after window (pool 96, windows of 192, a last window of 116), against one resident
    search of the dense tiles: heaps, tolerances, entered flags"""
    nchar, n, pool, window = 331, 500, 96, 192
    seqs = CL.near_identical_references(n + nq, nchar, 31)
    refs, qs = seqs[:n], [s.replace(b"N", b"A").replace(b"-", b"C") for s in seqs[n:]]
    dense, cf, _ = _files(tmp_path, refs, "win")
    with capi.Engine.from_query(O.Query(qs, ["q%d" % i for i in range(nq)]), nbest=4, max_pool=128) as eng:
        eng.db_reserve(n)
        eng.db_append_packed(*dense, n)
        ent = eng.search_resident(pool)
        want = eng.drain()
        eng.reset()
        eng.db_stage_reserve(window // 64)
        spans = [(a, min(n, a + window)) for a in range(0, n, window)]
        stage = lambda w: eng.db_stage_compact_at(w & 1, 0, *cf.stage_args(spans[w][0] // 64, (spans[w][1] - spans[w][0] + 63) // 64))
        stage(0)
        got_ent = []
        for w, (a, b) in enumerate(spans):
            eng.db_load_staged(w & 1, None, b - a)
            if w + 1 < len(spans):
                stage(w + 1)
            got_ent.append(eng.search_resident(pool, ordinal0=a))
        assert (spans[-1][1] - spans[-1][0]) % 64 != 0
        got = eng.drain()
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
        assert np.array_equal(np.concatenate(got_ent), ent) and ent.any()
        ms = eng.compact_ms()
        assert ms[0] > 0 and ms[1] > 0


# ---------------------------------------------------------------------------------------------------------------- command lines
NCOL = 1000
N_A, N_B = 230, 100                                          # a cut of the bundled alignment; an awkward set (both end inside a tile)


def _write_fasta(path, names, seqs):
    with open(path, "wb") as fh:
        for n, s in zip(names, seqs):
            fh.write(b">" + n.encode() + b"\n" + s + b"\n")


def _run(cmd, ok=True):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    assert (r.returncode == 0) == ok, (cmd, r.stderr[-2000:])
    return r.stderr.decode(errors="replace")


def _xz(prefix, suffix):
    return lzma.open(prefix + suffix, "rb").read()


@pytest.fixture(scope="module")
def cli(tmp_path_factory, bundled_db):
    d = tmp_path_factory.mktemp("compact_cli")
    names, seqs = bundled_db
    cols = np.linspace(400, 29400, NCOL).astype(np.int64)
    pick = lambda s: np.frombuffer(s, dtype=np.uint8)[cols].tobytes().upper()
    a, an = [pick(s) for s in seqs[:N_A]], list(names[:N_A])
    b, bn = [s.upper() for s in P.awkward_references(N_B, NCOL, 5)], ["awk%d" % i for i in range(N_B)]
    _write_fasta(d / "a.fa", an, a)
    _write_fasta(d / "b.fa", bn, b)
    f = {k: str(d / k) for k in ("a.fa", "b.fa", "q.fa", "dense.uvdb", "compact.uvdb", "dense_a.uvdb", "compact_a.uvdb", "compact_b.uvdb")}
    _run([UVAIAPACK, "-A", "0.9", "-o", f["dense.uvdb"], f["a.fa"], f["b.fa"]])
    log = _run([UVAIAPACK, "-A", "0.9", "--compact", "-o", f["compact.uvdb"], f["a.fa"], f["b.fa"]])
    assert "Packed %d of %d" % (N_A + N_B, N_A + N_B) in log
    _run([UVAIAPACK, "-A", "0.9", "-o", f["dense_a.uvdb"], f["a.fa"]])
    _run([UVAIAPACK, "-A", "0.9", "--compact", "-o", f["compact_a.uvdb"], f["a.fa"]])
    _run([UVAIAPACK, "-A", "0.9", "--compact", "-o", f["compact_b.uvdb"], f["b.fa"]])
    assert CL.file_version(f["compact.uvdb"]) == 2 and CL.file_version(f["dense.uvdb"]) == 1
    assert os.path.getsize(f["compact.uvdb"]) < os.path.getsize(f["dense.uvdb"])
    qs = [pick(s) for s in seqs[1000:1006]]
    qn = [an[70], bn[3]] + ["query%d" % i for i in range(4)]                  # two of them named like references: -x drops those
    _write_fasta(d / "q.fa", qn, qs)
    return d, f


@pytest.mark.parametrize("acgt", [[], ["--acgt"]])
@pytest.mark.parametrize("exclude", [[], ["-x"]])
@pytest.mark.parametrize("window", [[], ["--window", "128"]])
def test_uvaia_on_a_compact_file(cli, window, exclude, acgt):
    d, f = cli
    tag = "".join(x.strip("-") for x in window + exclude + acgt)
    base = [UVAIA, f["q.fa"], "-n", "4", "-A", "0.9", "-p", "64"] + window + exclude + acgt
    out_d, out_c = str(d / ("dense_" + tag)), str(d / ("compact_" + tag))
    _run(base + ["-o", out_d, "--packed", f["dense.uvdb"]])
    log = _run(base + ["-o", out_c, "--packed", f["compact.uvdb"]])
    for suffix in (".csv.xz", ".aln.xz"):
        want = _xz(out_d, suffix)
        assert len(want) > 500
        assert _xz(out_c, suffix) == want, suffix
    assert "Loaded %d packed sequences" % (N_A + N_B - (2 if exclude else 0)) in log


def test_uvaia_on_a_dense_and_a_compact_file(cli):
    d, f = cli
    base = [UVAIA, f["q.fa"], "-n", "4", "-A", "0.9", "-p", "64"]
    out_j, out_s, out_w = str(d / "mixed_joint"), str(d / "mixed_set"), str(d / "mixed_set_window")
    _run(base + ["-o", out_j, "--packed", f["dense.uvdb"]])
    _run(base + ["-o", out_s, "--packed", f["dense_a.uvdb"], "--packed", f["compact_b.uvdb"]])
    _run(base + ["-o", out_w, "--window", "128", "-x", "--packed", f["compact_a.uvdb"], "--packed", f["compact_b.uvdb"]])
    _run(base + ["-o", out_j + "_x", "-x", "--packed", f["dense.uvdb"]])
    for suffix in (".csv.xz", ".aln.xz"):
        assert _xz(out_s, suffix) == _xz(out_j, suffix), suffix
        assert _xz(out_w, suffix) == _xz(out_j + "_x", suffix), suffix


def test_merge_in_both_directions(cli):
    d, f = cli
    back, merged, mixed = str(d / "back.uvdb"), str(d / "merged_compact.uvdb"), str(d / "merged_mixed.uvdb")
    _run([UVAIAPACK, "--merge", "-o", back, f["compact.uvdb"]])                   # the way back to the dense file
    assert open(back, "rb").read() == open(f["dense.uvdb"], "rb").read()
    _run([UVAIAPACK, "--merge", "--compact", "-o", merged, f["compact_a.uvdb"], f["compact_b.uvdb"]])
    assert open(merged, "rb").read() == open(f["compact.uvdb"], "rb").read()
    _run([UVAIAPACK, "--merge", "--compact", "-o", mixed, f["dense_a.uvdb"], f["compact_b.uvdb"]])
    assert open(mixed, "rb").read() == open(f["compact.uvdb"], "rb").read()


@pytest.mark.parametrize("command", ["uvaia", "uvaiaball", "uvaiaclust"])
def test_refusals_name_the_way_back(cli, command):
    d, f = cli
    prefix = str(d / ("refused_" + command))
    cmd = {"uvaia": [UVAIA, f["q.fa"], "-A", "0.9", "--devices", "0,0", "-o", prefix, "--packed", f["dense_a.uvdb"], "--packed", f["compact_b.uvdb"]],
           "uvaiaball": [UVAIABALL, f["q.fa"], "-d", "40", "-o", prefix, "--packed", f["compact_b.uvdb"]],
           "uvaiaclust": [UVAIACLUST, "-d", "3", "-p", "8", "-o", prefix, "--packed", f["compact_b.uvdb"]]}[command]
    log = _run(cmd, ok=False)
    assert f["compact_b.uvdb"] in log and "uvaiapack --merge -o dense.uvdb" in log
    assert not [x for x in os.listdir(str(d)) if x.startswith("refused_" + command)]
