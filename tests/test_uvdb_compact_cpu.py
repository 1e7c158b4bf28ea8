"""The compact form of a packed database (version 2 of uvaia_amd/csrc/host/uvdb.h) on the host: writer, canonical encoding, base rule,
uvdb_open's checks, uvdb_expand_tiles and uvdb_unpack_reference.  No GPU."""
import numpy as np
import pytest

import compact_lib as CL
import packed_lib as PL


def _pack(seqs):
    up = [s.upper() for s in seqs]
    nchar = len(up[0])
    planes, non_n = PL.pack_tiles(up, nchar)
    return up, nchar, planes, non_n


def _write(tmp_path, seqs, name="c.uvdb", **kw):
    up, nchar, planes, non_n = _pack(seqs)
    path = tmp_path / name
    CL.write_compact(path, ["r%d" % i for i in range(len(up))], up, planes, non_n, **kw)
    return path, up, nchar, planes, non_n


def _acgt_row(nchar, shift=0):
    return bytes(b"ACGT"[(s + shift) & 3] for s in range(nchar))


def _with(row, a, b, ch):
    return row[:a] + ch * (b - a) + row[b:]


# ---------------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("kind", ["awkward", "near"])
@pytest.mark.parametrize("n_ref", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("nchar", [29, 128, 130, 1000])
def test_round_trip(tmp_path, nchar, n_ref, kind):
    seqs = PL.awkward_references(n_ref, nchar, 11 + n_ref) if kind == "awkward" else CL.near_identical_references(n_ref, nchar, 5 + n_ref)
    path, up, nchar, planes, non_n = _write(tmp_path, seqs)
    assert CL.file_version(path) == 2
    r = CL.Reader(path, nchar)
    try:
        assert r.dense_pointers_are_null()
        got, side = r.expand_tiles(0, planes.shape[0])
        assert np.array_equal(got, planes)                                        # byte for byte, zeros in the lanes past the end included
        want_side = CL.side_rows_canonical(planes, nchar)
        assert np.array_equal(side, want_side)
        if kind == "awkward" and nchar == 1000:
            assert want_side[:, 0].max() > CL.SIDE_LISTED                         # a list that is cut is among them
        for i in sorted({0, n_ref // 2, n_ref - 1}):
            assert r.unpack_reference(i) == up[i]
        if planes.shape[0] > 1:                                                   # a range that starts behind tile 0
            got1, side1 = r.expand_tiles(1, planes.shape[0] - 1)
            assert np.array_equal(got1, planes[1:]) and np.array_equal(side1, want_side[64:])
    finally:
        r.close()
    cf = CL.CompactFile(path)
    assert np.array_equal(cf.non_n, non_n) and cf.n_ref == n_ref


# ---------------------------------------------------------------------------------------------------------------- canonical encoding
def test_identical_rows_have_no_records(tmp_path):
    row = _acgt_row(1000)
    path, *_ = _write(tmp_path, [row] * 64)
    cf = CL.CompactFile(path)
    assert len(cf.heads) == 0 and len(cf.lits) == 0 and not cf.head_idx.any() and not cf.lit_idx.any()


def test_canonical_heads(tmp_path):
    nchar = 1000                                       # 32 words, the last one holds 8 sites; W4 = 8, no padding words
    row = _acgt_row(nchar)
    all_n = b"N" * nchar
    fill35 = _with(row, 96, 192, b"N")                 # words 3, 4, 5: across the word-group boundary at word 4
    first_last = _with(_with(row, 0, 1, b"R"), nchar - 1, nchar, b"N")          # word 0 (a literal) and the last real word
    sandwich = _with(_with(row, 320, 352, b"N"), 352, 353, b"N")                # word 10 a fill, one site of word 11 ...
    sandwich = _with(sandwich, 384, 416, b"-")                                  # ... and word 12 a fill again
    seqs = [row, row, row, row, all_n, fill35, first_last, sandwich]
    path, up, nchar, planes, _ = _write(tmp_path, seqs)
    cf = CL.CompactFile(path)
    assert cf.heads_of(0) == []                                                 # a row equal to the base
    assert cf.heads_of(4) == [(0, 32, 0, 0)]                                    # all N against an ACGT base: fills only
    assert cf.heads_of(5) == [(3, 3, 0, 0)]
    assert cf.heads_of(6) == [(0, 1, 1, 0), (31, 1, 1, 0)]                      # (the last word keeps 7 sites: a literal)
    assert cf.heads_of(7) == [(10, 1, 0, 0), (11, 1, 1, 0), (12, 1, 0, 0)]
    assert int(cf.lit_idx[7]) - int(cf.lit_idx[6]) == 2 and int(cf.lit_idx[8]) - int(cf.lit_idx[7]) == 1
    # the lanes past the last reference are all-zero rows against the base: one fill over the real words
    assert cf.heads_of(8) == [(0, 32, 0, 0)] and cf.heads_of(63) == [(0, 32, 0, 0)]
    r = CL.Reader(path, nchar)
    try:
        assert np.array_equal(r.expand_tiles(0, 1)[0], planes)
    finally:
        r.close()


def test_padding_words_never_appear(tmp_path):
    nchar = 130                                        # 5 real words in 8: words 5, 6, 7 are padding
    seqs = [_acgt_row(nchar)] * 3 + [b"N" * nchar, _with(_acgt_row(nchar), 128, 130, b"N")]
    path, *_ = _write(tmp_path, seqs)
    cf = CL.CompactFile(path)
    assert cf.heads_of(3) == [(0, 5, 0, 0)]
    assert cf.heads_of(4) == [(4, 1, 0, 0)]            # the last real word holds 2 sites, both N: all four planes zero, a fill
    for i in range(64):
        assert all(f + n <= 5 for f, n, _l, _c in cf.heads_of(i))
    assert all(cf.base_word(w) == (0, 0, 0, 0) for w in (5, 6, 7))


def test_fill_code_of_a_full_word(tmp_path):
    nchar = 128
    base = _acgt_row(nchar)
    seqs = [base] * 3 + [_with(base, 32, 96, b"A"), _with(base, 32, 64, b"R")]
    path, up, nchar, planes, _ = _write(tmp_path, seqs)
    cf = CL.CompactFile(path)
    assert cf.heads_of(3) == [(1, 2, 0, 1)]            # every site A: plane A all ones
    assert cf.heads_of(4) == [(1, 1, 0, 5)]            # every site R = {A, G}
    r = CL.Reader(path, nchar)
    try:
        assert np.array_equal(r.expand_tiles(0, 1)[0], planes)
        assert r.unpack_reference(4) == up[4]
    finally:
        r.close()


def test_fill_is_cut_at_2047_words(tmp_path):
    nchar = 70000                                      # 2188 words
    row = _acgt_row(nchar)
    path, up, nchar, planes, _ = _write(tmp_path, [row, row, b"N" * nchar, row])
    cf = CL.CompactFile(path)
    assert cf.heads_of(2) == [(0, 2047, 0, 0), (2047, 141, 0, 0)]
    assert cf.heads_of(0) == [] and cf.heads_of(3) == []
    r = CL.Reader(path, nchar)
    try:
        assert np.array_equal(r.expand_tiles(0, 1, side=False)[0], planes)
        assert r.unpack_reference(2) == up[2]
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- base rule
def test_base_is_the_strict_majority(tmp_path):
    nchar = 64
    seqs = [b"A" * 32 + b"C" * 32, b"A" * 32 + b"G" * 32, b"C" * 32 + b"T" * 32]
    path, *_ = _write(tmp_path, seqs)
    cf = CL.CompactFile(path)
    assert cf.base_word(0) == (0xFFFFFFFF, 0, 0, 0)    # A in two of three
    assert cf.base_word(1) == (0, 0, 0, 0)             # no base in more than half
    assert cf.heads_of(0) == [(1, 1, 0, 2)] and cf.heads_of(1) == [(1, 1, 0, 4)]
    assert cf.heads_of(2) == [(0, 1, 0, 2), (1, 1, 0, 8)]                        # two fills of different codes are two heads


def test_base_ignores_rows_behind_the_sample(tmp_path):
    nchar = 29
    n = CL.BASE_SAMPLE + 1
    seqs = [b"A" * nchar] * (CL.BASE_SAMPLE // 2) + [b"C" * nchar] * (CL.BASE_SAMPLE // 2) + [b"C" * nchar]
    assert len(seqs) == n
    path, up, nchar, planes, _ = _write(tmp_path, seqs, chunk_tiles=64)
    cf = CL.CompactFile(path)
    assert cf.base_word(0) == (0, 0, 0, 0)             # of the sample neither A nor C is in more than half; of all 4097 rows C would be
    r = CL.Reader(path, nchar)
    try:
        assert np.array_equal(r.expand_tiles(0, planes.shape[0], side=False)[0], planes)
        assert r.unpack_reference(n - 1) == up[n - 1]
    finally:
        r.close()
    # the same file whatever the pieces the tiles arrive in
    path2, *_ = _write(tmp_path, seqs, name="c2.uvdb")
    assert path.read_bytes() == path2.read_bytes()


# ---------------------------------------------------------------------------------------------------------------- damaged files
@pytest.fixture(scope="module")
def damage_file(tmp_path_factory):
    nchar = 1000
    row = _acgt_row(nchar)
    marked = _with(_with(_with(row, 64, 128, b"N"), 160, 161, b"R"), 320, 352, b"-")      # fill words 2-3, literal word 5, fill word 10
    path, *_ = _write(tmp_path_factory.mktemp("damage"), [row, row, row, marked, _with(row, 0, 32, b"N")])
    cf = CL.CompactFile(path)
    assert cf.heads_of(3) == [(2, 2, 0, 0), (5, 1, 1, 0), (10, 1, 0, 0)]
    return path, cf


def _patched(cf, off, value, dtype):
    raw = cf.raw.copy()
    raw[off:off + np.dtype(dtype).itemsize] = np.array([value], dtype=dtype).view(np.uint8)
    return raw


DAMAGE = ["index_decreases", "index_beyond_section", "lit_index_beyond_section", "no_words", "beyond_alignment", "overlap", "descending", "literal_mismatch",
          "truncated"]


@pytest.mark.parametrize("case", DAMAGE)
def test_damaged_file_is_refused(tmp_path, damage_file, case):
    path, cf = damage_file
    h3 = int(cf.head_idx[3])                            # the first head of reference 3
    at = lambda k: cf.off_heads + 4 * (h3 + k)
    raw = {
        "index_decreases": lambda: _patched(cf, cf.off_head_idx + 8 * 3, int(cf.head_idx[4]) + 1, np.uint64),
        "index_beyond_section": lambda: _patched(cf, cf.off_head_idx + 8 * cf.lanes, int(cf.head_idx[-1]) + (1 << 20), np.uint64),
        "lit_index_beyond_section": lambda: _patched(cf, cf.off_lit_idx + 8 * cf.lanes, int(cf.lit_idx[-1]) + (1 << 20), np.uint64),
        "no_words": lambda: _patched(cf, at(0), CL.head(2, 0, 0, 0), np.uint32),
        "beyond_alignment": lambda: _patched(cf, at(2), CL.head(31, 2, 0, 0), np.uint32),
        "overlap": lambda: _patched(cf, at(1), CL.head(3, 1, 1, 0), np.uint32),
        "descending": lambda: np.concatenate([cf.raw[:at(0)], cf.raw[at(2):at(3)], cf.raw[at(1):at(2)], cf.raw[at(0):at(1)], cf.raw[at(3):]]),
        "literal_mismatch": lambda: _patched(cf, at(0), CL.head(2, 2, 1, 0), np.uint32),
        "truncated": lambda: cf.raw[:len(cf.raw) - 16],
    }[case]()
    ok, msg = CL.try_open(path)
    assert ok, msg
    bad = tmp_path / "bad.uvdb"
    raw.tofile(str(bad))
    ok, msg = CL.try_open(bad)
    assert not ok and str(bad) in msg


# ---------------------------------------------------------------------------------------------------------------- the rest
def test_version_1_reads_as_before(tmp_path):
    seqs = [s.upper() for s in PL.awkward_references(70, 130, 3)]
    planes, non_n = PL.pack_tiles(seqs, 130)
    side = CL.side_rows_canonical(planes, 130)
    path = tmp_path / "d.uvdb"
    PL.write_uvdb(path, ["r%d" % i for i in range(70)], seqs, planes, non_n, side)
    assert CL.file_version(path) == 1
    r = CL.Reader(path, 130)
    try:
        assert not r.dense_pointers_are_null()
        assert all(r.unpack_reference(i) == seqs[i] for i in (0, 63, 64, 69))
        got, rows = r.expand_tiles(0, 2)
        assert np.array_equal(got, planes) and np.array_equal(rows, side)
    finally:
        r.close()


def test_compact_and_dense_hold_the_same_names_and_runs(tmp_path):
    seqs = [s.upper() for s in PL.awkward_references(70, 130, 4)]
    planes, non_n = PL.pack_tiles(seqs, 130)
    names = ["r%d" % i for i in range(70)]
    PL.write_uvdb(tmp_path / "d.uvdb", names, seqs, planes, non_n, CL.side_rows_canonical(planes, 130))
    CL.write_compact(tmp_path / "c.uvdb", names, seqs, planes, non_n)
    d, c = CL.Reader(tmp_path / "d.uvdb", 130), CL.Reader(tmp_path / "c.uvdb", 130)
    try:
        assert all(d.unpack_reference(i) == c.unpack_reference(i) == seqs[i] for i in range(70))
    finally:
        d.close(); c.close()


def test_alignment_beyond_the_limit_is_refused(tmp_path):
    assert not CL.create_compact(tmp_path / "x.uvdb", CL.MAX_NCHAR + 1)
    w = CL.create_compact(tmp_path / "y.uvdb", 1000)
    assert w and CL._lib().uvdb_close(w) == 0           # (an empty file is a file)
    assert CL.try_open(tmp_path / "y.uvdb")[0]
