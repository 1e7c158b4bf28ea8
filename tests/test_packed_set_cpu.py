"""Several packed databases as one stream, the host side (uvaia_amd/csrc/host/uvdb_set.h): the mapping of stream positions to files, the
pieces and selection entries of a range of kept positions against a numpy restatement, a set of one file against uvdb_window_span, the
chunks that go straight from a mapping, the refusals, and the same code driven by a stand-alone program under the address and
undefined-behaviour sanitizers.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import packed_lib as P
from uvaia_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "uvaia_amd", "csrc", "host")
NCHAR = 100


def _write(path, tag, n, nchar=NCHAR, ambiguity=0.5):
    """n references named <tag>_<i>; an empty file is written as well (every row of its text failed the -A filter)"""
    rng = np.random.default_rng(n + 7)
    seqs = [rng.choice(np.frombuffer(b"ACGTN-", dtype=np.uint8), size=nchar).tobytes() for _ in range(n)]
    L = P._lib()
    w = L.uvdb_create(str(path).encode(), nchar, P.tile_bytes(nchar), P.SIDE_ROW_INTS, ambiguity)
    assert w
    for i, s in enumerate(seqs):
        assert L.uvdb_add_reference(w, ("%s_%d" % (tag, i)).encode(), s) == 0
    if n:
        planes, non_n = P.pack_tiles(seqs, nchar)
        side = np.zeros((len(non_n), P.SIDE_ROW_INTS), dtype=np.int32)
        assert L.uvdb_add_tiles(w, planes.shape[0], planes.ctypes.data, non_n.ctypes.data, side.ctypes.data) == 0
    assert L.uvdb_close(w) == 0
    return seqs


# file sizes of a set: single files at the tile edges, files that end inside a tile, two whole tiles, a file that holds nothing at the end
SETS = [(1,), (63,), (64,), (65,), (5, 7, 60), (64, 64), (130, 1, 0), (0, 3, 0, 70), (1, 1, 1, 1, 200), (200,)]


def _restate(sizes, keep, a, b):
    """what uvdb_set_span promises, from the sizes alone: pieces (file, first tile, tiles, tile of the slot) and the selection"""
    first = np.concatenate([[0], np.cumsum(sizes)])
    idx = np.arange(a, b, dtype=np.int64) if keep is None else np.asarray(keep[a:b]).astype(np.int64)
    file_of = np.searchsorted(first, idx, side="right") - 1
    local = idx - first[file_of]
    pieces, sel, slot = [], np.zeros(len(idx), dtype=np.int64), 0
    for f in np.unique(file_of):
        mine = file_of == f
        t0, t1 = int(local[mine].min()) // 64, int(local[mine].max()) // 64 + 1
        pieces.append((int(f), t0, t1 - t0, slot))
        sel[mine] = slot * 64 + local[mine] - t0 * 64
        slot += t1 - t0
    return pieces, slot, sel


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("packed_set")
    out = {}
    for k, sizes in enumerate(SETS):
        paths = [d / ("s%d_%d.uvdb" % (k, f)) for f in range(len(sizes))]
        seqs = [_write(p, "s%df%d" % (k, f), n) for f, (p, n) in enumerate(zip(paths, sizes))]
        out[sizes] = (paths, seqs)
    return d, out


@pytest.mark.parametrize("sizes", SETS)
def test_stream_positions_names_and_text(sets, sizes):
    paths, seqs = sets[1][sizes]
    s = hostlib.UvdbSet(paths)
    total = sum(sizes)
    i = 0
    for f, n in enumerate(sizes):
        for r in range(n):
            assert s.locate(i) == (f, r)
            assert s.name(i) == "s%df%d_%d" % (SETS.index(sizes), f, r)
            assert s.unpack_reference(i, NCHAR) == seqs[f][r]
            assert s.non_n(i) == sum(c in b"ACGT" for c in seqs[f][r])
            i += 1
    assert i == total and s.locate(total) is None and s.name(total) is None
    s.close()


@pytest.mark.parametrize("sizes", SETS)
def test_pieces_and_selection_against_the_restatement(sets, sizes):
    paths, _ = sets[1][sizes]
    s = hostlib.UvdbSet(paths)
    total = sum(sizes)
    first = np.concatenate([[0], np.cumsum(sizes)])
    # kept lists: everything; holes at the file boundaries (first and last reference of every file); every third reference dropped
    at_edges = np.array([i for i in range(total) if i not in set(first) and i + 1 not in set(first)], dtype=np.uint64)
    thirds = np.array([i for i in range(total) if i % 3 != 1], dtype=np.uint64)
    for keep in (None, at_edges, thirds):
        n = total if keep is None else len(keep)
        ranges = [(0, n)] + [(a, min(n, a + w)) for w in (1, 50, 64, 100) for a in range(0, n, w)]
        ranges += [(a, b) for a in (3, 63, 66, 131) for b in (a + 1, a + 64, n) if a < b <= n]       # windows that start inside a file
        for a, b in ranges:
            if b <= a:
                continue
            got = s.span(keep, a, b)
            assert got is not None, (sizes, a, b)
            pieces, slot, sel = _restate(sizes, keep, a, b)
            assert got[0] == pieces and got[1] == slot and np.array_equal(got[2], sel), (sizes, keep is None, a, b)
            assert np.all(np.diff(sel) > 0) and sel[-1] < slot * 64
    if sizes == (1, 1, 1, 1, 200):                           # one window over five files, three of them inside it
        assert [p[0] for p in s.span(None, 1, 4)[0]] == [1, 2, 3]
        assert len(s.span(None, 0, total)[0]) == 5 and s.span(None, 0, total, max_pieces=4) is None
    if sizes == (130, 1, 0):                                 # the file that holds nothing gives no piece
        assert [p[0] for p in s.span(None, 100, 131)[0]] == [0, 1]
    assert s.span(None, 0, total + 1) is None and s.span(None, 2, 2) is None
    if total > 3:
        assert s.span(np.array([2, 1, 3], dtype=np.uint64), 0, 3) is None          # not increasing
        assert s.span(np.array([1, total], dtype=np.uint64), 0, 2) is None         # outside the stream
    s.close()


def _kept_lists(sizes):
    """the kept lists of test_pieces_and_selection_against_the_restatement"""
    total = sum(sizes)
    first = set(np.concatenate([[0], np.cumsum(sizes)]).tolist())
    at_edges = np.array([i for i in range(total) if i not in first and i + 1 not in first], dtype=np.uint64)
    thirds = np.array([i for i in range(total) if i % 3 != 1], dtype=np.uint64)
    return (None, at_edges, thirds)


@pytest.mark.parametrize("sizes", [s for s in SETS if len(s) == 1])
def test_a_set_of_one_file_plans_what_uvdb_window_span_plans(sets, sizes):
    """one piece (0, first_tile, n_tiles, 0) with the tiles and the selection uvdb_window_span gives for the same keep, a, b"""
    L = hostlib.load_library()
    U64 = C.c_uint64
    L.uvdb_window_span.restype = C.c_int
    L.uvdb_window_span.argtypes = [C.POINTER(U64), U64, U64, C.POINTER(U64), C.POINTER(U64), C.POINTER(C.c_int)]
    paths, _ = sets[1][sizes]
    s = hostlib.UvdbSet(paths)
    checked = 0
    for keep in _kept_lists(sizes):
        n = sizes[0] if keep is None else len(keep)
        ranges = [(0, n)] + [(a, min(n, a + w)) for w in (1, 50, 64, 100) for a in range(0, n, w)]
        ranges += [(a, b) for a in (3, 63, 66, 131) for b in (a + 1, a + 64, n) if a < b <= n]
        for a, b in ranges:
            if b <= a:
                continue
            arr = None if keep is None else keep.ctypes.data_as(C.POINTER(U64))
            t0, nt = U64(0), U64(0)
            sel = np.full(b - a, -1, dtype=np.int32)
            assert L.uvdb_window_span(arr, a, b, C.byref(t0), C.byref(nt), sel.ctypes.data_as(C.POINTER(C.c_int))) == 0
            pieces, slot, got = s.span(keep, a, b)
            assert pieces == [(0, t0.value, nt.value, 0)] and slot == nt.value and np.array_equal(got, sel), (sizes, keep is None, a, b)
            checked += 1
    assert checked >= 3
    s.close()


def _direct(sizes, keep, a, b, n, store):
    """what uvdb_set_direct_tiles promises, from the sizes alone: (file, first tile) of a range that is whole tiles of one file behind
    whole tiles, None for any other"""
    first = np.concatenate([[0], np.cumsum(sizes)])
    if keep is not None or b <= a or b > n or store % 64:
        return None
    f = int(np.searchsorted(first, a, side="right")) - 1
    local = a - int(first[f])
    if local % 64 or b > first[f + 1]:                       # not at lane 0 of a tile, or not in one file
        return None
    if (b - a) % 64 and b != n:                              # a partly filled tile anywhere but at the end of the stream
        return None
    return f, local // 64


@pytest.mark.parametrize("sizes", SETS)
def test_direct_tiles_against_the_restatement(sets, sizes):
    paths, _ = sets[1][sizes]
    s = hostlib.UvdbSet(paths)
    total = sum(sizes)
    yes = 0
    for keep in (None, _kept_lists(sizes)[2]):
        n = total if keep is None else len(keep)
        for chunk in (64, 100, 128):
            for store in (0, 64, 70):
                for a in range(0, n, chunk):
                    b = min(n, a + chunk)
                    got = s.direct_tiles(keep, a, b, n, store)
                    assert got == _direct(sizes, keep, a, b, n, store), (sizes, keep is None, chunk, store, a, b)
                    yes += got is not None
        assert s.direct_tiles(keep, 0, 0, n, 0) is None and s.direct_tiles(keep, 64, 64, n, 0) is None          # an empty range
        assert s.direct_tiles(keep, 0, n + 1, n + 1, 0) is None and s.direct_tiles(keep, n, n + 64, n + 64, 0) is None      # past the stream
    if len(sizes) == 1 or sizes[0] >= 64:                    # the first chunk into an empty store, at the least
        assert yes > 0
    if sizes == (200,):                                      # one file without -x: every chunk, the last partly filled one too
        assert [s.direct_tiles(None, a, min(200, a + 64), 200, a) for a in range(0, 200, 64)] == [(0, 0), (0, 1), (0, 2), (0, 3)]
    if sizes == (130, 1, 0):                                 # a set: the leading chunks of the first file, nothing behind the cut tile
        assert [s.direct_tiles(None, a, min(131, a + 64), 131, a) for a in range(0, 131, 64)] == [(0, 0), (0, 1), None]
    s.close()


def test_files_that_do_not_agree_are_refused_by_name(sets, tmp_path):
    paths, _ = sets[1][(5, 7, 60)]
    other_nchar, other_a = tmp_path / "wide.uvdb", tmp_path / "tight.uvdb"
    _write(other_nchar, "w", 3, nchar=129)
    _write(other_a, "t", 3, ambiguity=0.25)
    with pytest.raises(ValueError) as ei:
        hostlib.UvdbSet([paths[0], paths[1], other_nchar])
    msg = str(ei.value)
    assert str(other_nchar) in msg and str(paths[0]) in msg and "129 sites" in msg and "100 sites" in msg
    with pytest.raises(ValueError) as ei:
        hostlib.UvdbSet([paths[0], other_a, paths[1]])
    msg = str(ei.value)
    assert str(other_a) in msg and str(paths[0]) in msg and "-A 0.25" in msg and "-A 0.5" in msg and "uvaiapack --merge -A" in msg
    s = hostlib.UvdbSet([paths[0], other_a, paths[1]], flags=hostlib.UvdbSet.ANY_AMBIGUITY)       # the merge tool reads them all the same
    assert s.locate(5) == (1, 0) and s.locate(8) == (2, 0)
    s.close()
    with pytest.raises(ValueError) as ei:
        hostlib.UvdbSet([paths[0], tmp_path / "missing.uvdb"])
    assert "missing.uvdb" in str(ei.value)
    with pytest.raises(ValueError):
        hostlib.UvdbSet([])


def test_uvdb_set_under_the_sanitizers(tmp_path):
    """tests/uvdb_set_driver.c with uvdb.c and uvdb_set.c, all built with -fsanitize=address,undefined: a stand-alone host program"""
    exe = tmp_path / "uvdb_set_driver"
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-I", HOST, os.path.join(ROOT, "tests", "uvdb_set_driver.c"), os.path.join(HOST, "uvdb_set.c"), os.path.join(HOST, "uvdb.c"), "-o", str(exe)])
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([str(exe), str(work)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    assert b"uvdb_set driver: ok" in r.stdout
