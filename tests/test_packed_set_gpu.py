"""Several packed databases as one stream, on a GPU box: the device-side append of staged lanes at any position of the resident store
(uvaia_gpu_db_append_staged, append_lanes_kernel), pieces of a staging slot (uvaia_gpu_db_stage_packed_at), and the command lines built
on them: a repeated --packed of uvaia, uvaiaball and uvaiaclust against their text runs, `uvaiapack --merge` against the joint pack."""
import itertools
import lzma
import os
import subprocess

import numpy as np
import pytest

import fixtures as F
import oracle_lib as O
import packed_lib as P
from uvaia_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIA = os.path.join(ROOT, "bin", "uvaia")
UVAIABALL = os.path.join(ROOT, "bin", "uvaiaball")
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")

SIZES = (1, 5, 63, 64, 65)
SPLITS = list(itertools.product(SIZES, repeat=2)) + list(itertools.product(SIZES, repeat=3))
N_POOL = 3 * 65 + 64 + 7                                     # the largest split, shifted by up to a tile, and a tail
_cache = {}


def _pool(nchar):
    """five queries and N_POOL references that hold every IUPAC code (side rows are not empty) and runs of - ? N; their upper-case text
    and interchange tiles out of a default-mode context"""
    if nchar not in _cache:
        root = F.random_acgt(nchar, 11)
        qs = []
        for i in range(5):
            s = bytearray(root)
            s[(17 * i + 3) % nchar] = b"ACGT"[(b"ACGT".index(s[(17 * i + 3) % nchar]) + 1) % 4]
            qs.append(bytes(s))
        qn = ["q%d" % i for i in range(len(qs))]
        refs = P.awkward_references(N_POOL, nchar, seed=nchar)
        with capi.Engine.from_query(O.Query(qs, qn), nbest=2, max_pool=64) as eng:
            eng.db_reserve(len(refs))
            eng.db_append(refs)
            tiles = eng.db_export()
        upper = [r.upper() for r in refs]
        assert tiles[2][:N_POOL, 0].max() > 0                 # some side row lists a partially ambiguous word
        assert any(b"--" in r for r in upper) and any(b"??" in r for r in upper) and any(b"NN" in r for r in upper)
        _cache[nchar] = (qs, qn, upper, tiles)
    return _cache[nchar]


def _compact(tiles, rows):
    """host-side compaction of rows[] of the tiles: ceil(len / 64) tiles, zero past the last"""
    planes, non_n, side = tiles
    rows = np.asarray(rows, dtype=np.int64)
    nt = max((len(rows) + 63) // 64, 1)
    src = planes.reshape(planes.shape[0], -1, 64, 16)        # [tile][word group x plane][lane][16 bytes]
    out = np.zeros((nt,) + src.shape[1:], dtype=np.uint8)
    out_n = np.zeros(nt * 64, dtype=np.int32)
    out_s = np.zeros((nt * 64, side.shape[1]), dtype=np.int32)
    k = np.arange(len(rows))
    out[k // 64, :, k % 64, :] = src[rows // 64, :, rows % 64, :]
    out_n[:len(rows)] = non_n[rows]
    out_s[:len(rows)] = side[rows]
    return out.reshape(nt, -1), out_n, out_s


def _variants(split):
    """nothing dropped, and for every group of the split -- the one that starts the database and the last one included -- its first row,
    its last row and the whole of it dropped"""
    return [("all", -1)] + [(what, g) for g in range(len(split)) for what in ("first", "last", "group")]


CASES = [(split, variant) for split in SPLITS for variant in _variants(split)]


def _groups(split, variant, shift):
    """[(first row of the pool, rows of the group, kept rows)]: group g starts `shift` rows into the pool (its lanes differ from the
    destination's); variant = (what, g) drops the first row, the last row or the whole of group g"""
    what, which = variant
    out, at = [], shift
    for g, size in enumerate(split):
        kept = list(range(at, at + size))
        if g == which and what == "first":
            kept = kept[1:]
        if g == which and what == "last":
            kept = kept[:-1]
        if g == which and what == "group":
            kept = []
        out.append((at, size, kept))
        at += size
    return out


def _append_groups(eng, tiles, groups):
    """every group staged as the whole tiles of the pool that hold it, its kept rows appended behind what is resident"""
    planes, non_n, side = tiles
    for g, (at, size, kept) in enumerate(groups):
        t0, t1 = at // 64, (at + size - 1) // 64 + 1
        eng.db_stage_packed(g & 1, planes[t0:t1], non_n[t0 * 64:t1 * 64], side[t0 * 64:t1 * 64], t1 - t0)
        sel = [r - t0 * 64 for r in kept]
        before = eng.db_size()
        eng.db_append_staged(g & 1, None if sel == list(range(len(sel))) else sel, len(sel))
        assert eng.db_size() == before + len(kept)


@pytest.mark.parametrize("nchar", [100, 128, 129, 1000])
def test_append_staged_is_one_append_packed(nchar):
    qs, qn, upper, tiles = _pool(nchar)
    with capi.Engine.from_query(O.Query(qs, qn), nbest=2, max_pool=128) as eng:
        eng.db_reserve(N_POOL)
        eng.db_stage_reserve(5)
        for split, variant in CASES:
            shift = (7 * len(split) + split[0]) % 64
            groups = _groups(split, variant, shift)
            rows = [r for _, _, kept in groups for r in kept]
            eng.db_clear()
            if rows:
                eng.db_append_packed(*_compact(tiles, rows), len(rows))
            want = eng.db_export() if rows else None
            eng.db_clear()
            _append_groups(eng, tiles, groups)
            assert eng.db_size() == len(rows)
            if rows:
                for g, w, what in zip(eng.db_export(), want, ("planes", "non_n", "side rows")):
                    assert np.array_equal(g, w), (nchar, split, variant, what)
                pad = len(rows) % 64
                if pad:                                          # the padding lanes of the last tile read as zero
                    got = eng.db_export()
                    assert not got[0].reshape(got[0].shape[0], -1, 64, 16)[-1, :, pad:, :].any() and not got[1][len(rows):].any() and not got[2][len(rows):].any()


def test_append_staged_behind_text_rows_and_refusals():
    """behind rows that came as text (the first tile holds resident lanes written by another kernel), and what is refused"""
    qs, qn, upper, tiles = _pool(129)
    with capi.Engine.from_query(O.Query(qs, qn), nbest=2, max_pool=128) as eng:
        eng.db_reserve(N_POOL)
        with pytest.raises(capi.GpuError) as ei:             # nothing staged yet
            eng.db_append_staged(0, None, 1)
        assert ei.value.code == -6
        eng.db_stage_reserve(4)
        eng.db_append(upper[:37])
        eng.db_stage_packed(0, tiles[0][:4], tiles[1][:256], tiles[2][:256], 4)
        eng.db_append_staged(0, list(range(37, 200)), 163)
        want = _compact(tiles, list(range(200)))
        for g, w in zip(eng.db_export(), want):
            assert np.array_equal(g, w)
        for bad in ([-1], [0, 256], [1 << 30]):              # refused before anything is launched: the database as before
            with pytest.raises(capi.GpuError) as ei:
                eng.db_append_staged(0, bad, len(bad))
            assert ei.value.code == -1
        with pytest.raises(capi.GpuError) as ei:
            eng.db_append_staged(2, None, 1)
        assert ei.value.code == -1
        with pytest.raises(capi.GpuError) as ei:             # beyond the reserved capacity
            eng.db_append_staged(0, None, 256)
        assert ei.value.code == -6
        assert eng.db_size() == 200
        for g, w in zip(eng.db_export(), want):
            assert np.array_equal(g, w)
        rows = eng.db_unpack_rows([0, 36, 37, 199])          # the text of the whole resident database
        assert rows == [P.decode_reference(tiles[0], i, 129) for i in (0, 36, 37, 199)]


def _whole_tiles_then_staged(eng, tiles, rows, whole):
    """the resident load of a stream whose leading chunk goes as whole host tiles: one append_packed of rows[:whole], the tiles of the
    pool that hold the others staged and their lanes (which are not the destination's) appended"""
    planes, non_n, side = tiles
    eng.db_append_packed(*_compact(tiles, rows[:whole]), whole)
    t0, t1 = rows[whole] // 64, rows[-1] // 64 + 1
    eng.db_stage_packed(0, planes[t0:t1], non_n[t0 * 64:t1 * 64], side[t0 * 64:t1 * 64], t1 - t0)
    sel = [r - t0 * 64 for r in rows[whole:]]
    assert sel[0] % 64 != 0                                  # a lane shift: destination lane 0 reads another lane of the slot
    eng.db_append_staged(0, sel, len(sel))
    assert eng.db_size() == len(rows)


@pytest.mark.parametrize("whole,rest", [(128, 70), (64, 1)])
def test_append_staged_behind_append_packed_is_one_append_packed(whole, rest):
    qs, qn, upper, tiles = _pool(129)
    rows = list(range(5, 5 + whole + rest))
    with capi.Engine.from_query(O.Query(qs, qn), nbest=2, max_pool=128) as eng:
        eng.db_reserve(N_POOL)
        eng.db_stage_reserve(3)
        eng.db_append_packed(*_compact(tiles, rows), len(rows))
        want = eng.db_export()
        eng.db_clear()
        _whole_tiles_then_staged(eng, tiles, rows, whole)
        got = eng.db_export()
        for g, w, what in zip(got, want, ("planes", "non_n", "side rows")):
            assert np.array_equal(g, w), (whole, rest, what)
        pad = len(rows) % 64                                 # the padding lanes of the last tile read as zero
        assert pad and not got[0].reshape(got[0].shape[0], -1, 64, 16)[-1, :, pad:, :].any() and not got[1][len(rows):].any() and not got[2][len(rows):].any()


@pytest.mark.parametrize("whole,rest", [(128, 70), (64, 1)])
def test_append_staged_behind_append_packed_acgt_context(whole, rest):
    """the same two calls in an --acgt context: the heaps of a search against one append_packed load (append_packed keeps no four-plane
    image, so there is no text of the rows to compare)"""
    qs, qn, upper, tiles = _pool(129)
    rows = list(range(5, 5 + whole + rest))
    with capi.Engine.from_query(O.Query(qs, qn, acgt=True), nbest=4, max_pool=64) as eng:
        eng.db_reserve(N_POOL)
        eng.db_stage_reserve(3)
        eng.db_append_packed(*_compact(tiles, rows), len(rows))
        ent = eng.search_resident(64)
        want = eng.drain()
        eng.reset(); eng.db_clear()
        _whole_tiles_then_staged(eng, tiles, rows, whole)
        got_ent = eng.search_resident(64)
        got = eng.drain()
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), (whole, rest)
        assert np.array_equal(got_ent, ent) and ent.any()


@pytest.mark.parametrize("nchar", [100, 128, 129, 1000])
def test_append_staged_acgt_context(nchar):
    """an --acgt context re-codes while appending: the heaps of a search and the text of every row against one append_packed load"""
    qs, qn, upper, tiles = _pool(nchar)
    text = [P.decode_reference(tiles[0], i, nchar) for i in range(N_POOL)]
    with capi.Engine.from_query(O.Query(qs, qn, acgt=True), nbest=4, max_pool=64) as eng:
        eng.db_reserve(N_POOL)
        eng.db_stage_reserve(5)
        for split, variant in CASES:
            shift = (7 * len(split) + split[0]) % 64
            groups = _groups(split, variant, shift)
            rows = [r for _, _, kept in groups for r in kept]
            if not rows:
                continue
            eng.reset(); eng.db_clear()
            eng.db_append_packed(*_compact(tiles, rows), len(rows))
            ent = eng.search_resident(64)
            want = eng.drain()
            eng.reset(); eng.db_clear()
            _append_groups(eng, tiles, groups)
            got_ent = eng.search_resident(64)
            got = eng.drain()
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), (nchar, split, variant)
            assert np.array_equal(got_ent, ent), (nchar, split, variant)
            assert eng.db_unpack_rows(list(range(len(rows)))) == [text[r] for r in rows], (nchar, split, variant)


def test_acgt_image_ends_with_rows_that_were_not_staged():
    """the four-plane image an --acgt context decodes from covers rows that came through load_staged / append_staged only: after a clear
    and rows that came as text, an append of staged rows must not make the old window's image stand for them"""
    qs, qn, upper, tiles = _pool(129)
    text = [P.decode_reference(tiles[0], i, 129) for i in range(N_POOL)]
    with capi.Engine.from_query(O.Query(qs, qn, acgt=True), nbest=2, max_pool=128) as eng:
        eng.db_reserve(N_POOL)
        eng.db_stage_reserve(4)
        eng.db_stage_packed(0, tiles[0][:4], tiles[1][:256], tiles[2][:256], 4)
        eng.db_load_staged(0, None, 100)
        assert eng.db_unpack_rows([0, 99]) == [text[0], text[99]]
        eng.db_clear()
        eng.db_append(upper[100:200])                        # as many rows as the window held, other rows
        with pytest.raises(capi.GpuError) as ei:
            eng.db_unpack_rows([0])
        assert ei.value.code == -6
        eng.db_append_staged(0, list(range(200, 230)), 30)
        assert eng.db_size() == 130
        with pytest.raises(capi.GpuError) as ei:             # rows 0..99 have no image: refused, not decoded from the old window
            eng.db_unpack_rows([0])
        assert ei.value.code == -6
        eng.db_clear()                                       # from an empty database on the image is whole again
        eng.db_append_staged(0, list(range(3, 80)), 77)
        eng.db_append_staged(0, list(range(200, 230)), 30)
        assert eng.db_unpack_rows([0, 76, 77, 106]) == [text[3], text[79], text[200], text[229]]
        eng.db_drop_tiles(1)                                 # the tiles move, the image does not
        with pytest.raises(capi.GpuError) as ei:
            eng.db_unpack_rows([0])
        assert ei.value.code == -6


def test_stage_packed_at_pieces_are_one_staging():
    qs, qn, upper, tiles = _pool(129)
    planes, non_n, side = tiles
    with capi.Engine.from_query(O.Query(qs, qn), nbest=2, max_pool=128) as eng:
        eng.db_stage_reserve(4)
        eng.db_stage_packed(0, planes[:4], non_n[:256], side[:256], 4)
        eng.db_load_staged(0, None, 250)
        want = eng.db_export()
        for k in (1, 3):
            eng.db_stage_packed_at(1, 0, planes[:k], non_n[:k * 64], side[:k * 64], k)
            with pytest.raises(capi.GpuError) as ei:         # the slot holds k tiles so far
                eng.db_load_staged(1, None, k * 64 + 1)
            assert ei.value.code == -1
            eng.db_stage_packed_at(1, k, planes[k:4], non_n[k * 64:256], side[k * 64:256], 4 - k)
            eng.db_load_staged(1, None, 250)
            for g, w in zip(eng.db_export(), want):
                assert np.array_equal(g, w), k
        sel = list(range(1, 21)) + list(range(65, 85)) + list(range(192, 255))      # stage_packed is stage_packed_at at tile 0
        eng.db_stage_packed(0, planes[:4], non_n[:256], side[:256], 4)
        eng.db_load_staged(0, sel, len(sel))
        want = eng.db_export()
        eng.db_stage_packed_at(1, 0, planes[:4], non_n[:256], side[:256], 4)
        eng.db_load_staged(1, sel, len(sel))
        for g, w, c in zip(eng.db_export(), want, _compact(tiles, sel)):
            assert np.array_equal(g, w) and np.array_equal(g, c)
        for off, nt in ((4, 1), (5, 0), (2, 3), (1 << 40, 1)):      # a piece that ends beyond the reserved tiles
            with pytest.raises(capi.GpuError) as ei:
                eng.db_stage_packed_at(1, off, planes[:nt], non_n[:nt * 64], side[:nt * 64], nt)
            assert ei.value.code == -6, (off, nt)
        eng.db_stage_packed_at(1, 4, planes[:0], non_n[:0], side[:0], 0)       # an empty piece at the end is not


# ---------------------------------------------------------------------------------------------------------------- command lines
NCOL = 1000
SIZES_CLI = (70, 1, 100)                                     # a file that ends inside its second tile, a file of one row, one that ends inside a tile
HEAVY = (10, 70, 170)                                        # one row per file that -A 0.9 keeps and -A 0.5 drops (600 of 1000 sites are N)


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
    d = tmp_path_factory.mktemp("packed_set_cli")
    names, seqs = bundled_db
    cols = np.linspace(400, 29400, NCOL).astype(np.int64)
    pick = lambda s: np.frombuffer(s, dtype=np.uint8)[cols].tobytes().upper()
    n = sum(SIZES_CLI)
    refs, rnames = [pick(s) for s in seqs[:n]], list(names[:n])
    for i in HEAVY:
        refs[i] = b"N" * 600 + refs[i][600:]
    texts, packed, at = [], [], 0
    for f, size in enumerate(SIZES_CLI):
        fa, db = d / ("%s.fa" % "abc"[f]), d / ("%s.uvdb" % "abc"[f])
        _write_fasta(fa, rnames[at:at + size], refs[at:at + size])
        _run([UVAIAPACK, "-A", "0.9", "-o", str(db), str(fa)])
        texts.append(str(fa)); packed.append(str(db))
        at += size
    _run([UVAIAPACK, "-A", "0.9", "-o", str(d / "abc.uvdb")] + texts)
    qs = [pick(s) for s in seqs[1000:1006]]
    qn = [rnames[70], rnames[76]] + ["query%d" % i for i in range(4)]        # named like the row of file 2 and like a row of file 3
    _write_fasta(d / "q.fa", qn, qs)
    return d, texts, packed, str(d / "abc.uvdb"), rnames, refs


@pytest.mark.parametrize("extra,set_only", [([], []), (["-x"], []), (["--acgt"], []), (["-p", "64"], ["--window", "64"]), ([], ["--devices", "0,0"]),
                                            (["-x", "-p", "64"], ["--window", "64"])])
def test_uvaia_over_three_packed_files(cli, extra, set_only):
    d, texts, packed, joint, rnames, refs = cli
    tag = "".join(x.strip("-").replace(",", "") for x in extra + set_only)
    base = [UVAIA, str(d / "q.fa"), "-n", "4", "-A", "0.9"] + extra
    out = {k: str(d / ("%s_%s" % (k, tag))) for k in ("text", "joint", "set")}
    _run(base + ["-o", out["text"]] + [x for t in texts for x in ("-r", t)])
    _run(base + ["-o", out["joint"], "--packed", joint])
    log = _run(base + ["-o", out["set"]] + set_only + [x for p in packed for x in ("--packed", p)])
    windowed = "--window" in set_only                        # the joint file a window at a time too: a set of one, windowed
    if windowed:
        out["joint_window"] = str(d / ("joint_window_" + tag))
        _run(base + ["-o", out["joint_window"], "--packed", joint] + set_only)
    for suffix in (".csv.xz", ".aln.xz"):
        want = _xz(out["text"], suffix)
        assert len(want) > 500
        assert _xz(out["joint"], suffix) == want, suffix
        assert _xz(out["set"], suffix) == want, suffix
        if windowed:
            assert _xz(out["joint_window"], suffix) == want, suffix
    assert "Loaded %d packed sequences from 3 files" % (sum(SIZES_CLI) - (2 if "-x" in extra else 0)) in log
    if "-x" in extra:
        assert " 2 reference sequences already present" in log


def test_uvaiaball_over_three_packed_files(cli):
    d, texts, packed, joint, rnames, refs = cli
    out_t, out_p = str(d / "ball_text"), str(d / "ball_set")
    _run([UVAIABALL, str(d / "q.fa"), "-d", "40", "-o", out_t] + [x for t in texts for x in ("-r", t)])
    log = _run([UVAIABALL, str(d / "q.fa"), "-d", "40", "-p", "64", "-o", out_p] + [x for p in packed for x in ("--packed", p)])
    want = _xz(out_t, ".aln.xz")
    assert _xz(out_p, ".aln.xz") == want
    assert 0 < want.count(b">") < sum(SIZES_CLI)
    assert "Loaded %d packed sequences from 3 files" % sum(SIZES_CLI) in log


def test_uvaiaclust_over_three_packed_files(cli):
    d, texts, packed, joint, rnames, refs = cli
    out_t, out_p = str(d / "clust_text"), str(d / "clust_set")
    _run([UVAIACLUST, "-d", "3", "-p", "8", "-o", out_t] + texts)
    _run([UVAIACLUST, "-d", "3", "-p", "8", "-o", out_p] + [x for p in packed for x in ("--packed", p)])
    for suffix in (".csv.xz", ".aln.xz"):
        want = _xz(out_t, suffix)
        assert _xz(out_p, suffix) == want, suffix
    assert 1 < _xz(out_t, ".aln.xz").count(b">") <= sum(SIZES_CLI)


def test_uvaiapack_merge_is_the_joint_pack(cli):
    d, texts, packed, joint, rnames, refs = cli
    merged = str(d / "merged.uvdb")
    log = _run([UVAIAPACK, "--merge", "-o", merged] + packed)
    assert open(merged, "rb").read() == open(joint, "rb").read()
    assert "Merged %d of %d sequences" % (sum(SIZES_CLI), sum(SIZES_CLI)) in log and "-A 0.9" in log
    # a tighter -A: the heavy row of every file goes (the only row of the second file with them), as from the texts
    tight_joint, tight_merged = str(d / "abc_tight.uvdb"), str(d / "merged_tight.uvdb")
    _run([UVAIAPACK, "-A", "0.5", "-o", tight_joint] + texts)
    log = _run([UVAIAPACK, "--merge", "-A", "0.5", "-o", tight_merged] + packed)
    assert "Merged %d of %d sequences" % (sum(SIZES_CLI) - len(HEAVY), sum(SIZES_CLI)) in log
    assert open(tight_merged, "rb").read() == open(tight_joint, "rb").read()
    for f, i in enumerate(HEAVY):                            # one row of every file was dropped
        lo, hi = sum(SIZES_CLI[:f]), sum(SIZES_CLI[:f + 1])
        assert lo <= i < hi and sum(c != ord("N") for c in refs[i]) < 500
    # the merged file in two steps, and a file merged with itself alone
    ab, ab_c = str(d / "ab.uvdb"), str(d / "ab_c.uvdb")
    _run([UVAIAPACK, "--merge", "-o", ab] + packed[:2])
    _run([UVAIAPACK, "--merge", "-o", ab_c, ab, packed[2]])
    assert open(ab_c, "rb").read() == open(joint, "rb").read()
    # a looser -A than an input's is refused; so are inputs of different -A without one
    log = _run([UVAIAPACK, "--merge", "-A", "0.95", "-o", str(d / "refused.uvdb")] + packed, ok=False)
    assert "looser" in log and packed[0] in log
    log = _run([UVAIAPACK, "--merge", "-o", str(d / "refused.uvdb"), packed[0], tight_joint], ok=False)
    assert "uvaiapack --merge -A" in log and packed[0] in log and tight_joint in log
    log = _run([UVAIA, str(d / "q.fa"), "-A", "0.9", "-o", str(d / "refused"), "--packed", packed[0], "--packed", tight_joint], ok=False)
    assert "uvaiapack --merge -A" in log
