"""uvaia_gpu_db_pairs and uvaia_gpu_db_pairs_within against the oracle's two kernels: every counter of every pair, exactly, at the lane,
tile, word, word-group, window and launch edges; however the rows entered the database; the list of the pairs within a distance; refusals;
and that a search before and after sees the same database."""
import numpy as np
import pytest

import packed_lib as P
import pair_dist as D
from uvaia_amd import capi

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6


def engine(nchar, acgt=False, reserve=256):
    eng = capi.Engine.from_query(D.dummy_query(nchar, acgt), nbest=4, max_pool=64)
    eng.db_reserve(reserve)
    return eng


def loaded(name):
    seqs, nchar = D.case(name)
    eng = engine(nchar, reserve=len(seqs))
    eng.db_append(seqs)
    return eng


def check_all(eng, expect, trim=0, rows=None, cols=None):
    """both forms (and the other row-tile height) of a rectangle against expect[rows, cols]"""
    n = expect.shape[0]
    r0, nr = rows or (0, n)
    c0, nc = cols or (0, n)
    want = expect[r0:r0 + nr, c0:c0 + nc]
    got = eng.db_pairs(rows=(r0, nr), cols=(c0, nc), trim=trim, what=capi.PAIRS_COUNTS)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "counters differ at (row, col, counter) %r ... got %r want %r" % (bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    for what in (capi.PAIRS_SNP, capi.PAIRS_SNP_ALT):
        got = eng.db_pairs(rows=(r0, nr), cols=(c0, nc), trim=trim, what=what)
        assert np.array_equal(got, D.snp(want)), what


# ---- lane and tile edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_database_sizes_around_a_tile(n):
    name = "awkward%dx129" % n
    with loaded(name) as eng:
        check_all(eng, D.oracle_counts(name))


@pytest.fixture(scope="module")
def synth():
    with loaded("synth130") as eng:
        yield eng


@pytest.mark.parametrize("rows, cols", [((5, 70), (60, 10)), ((64, 66), (0, 64)), ((129, 1), (129, 1)), ((0, 130), (63, 2)), ((31, 34), (0, 130))])
def test_rectangles_that_are_not_tile_aligned(synth, rows, cols):
    check_all(synth, D.oracle_counts("synth130"), rows=rows, cols=cols)


def test_leading_dimension_leaves_the_padding_untouched(synth):
    want = D.oracle_counts("synth130")[5:75, 60:70]
    out = np.full((70, 13), -7, dtype=np.int32)
    synth.db_pairs(rows=(5, 70), cols=(60, 10), out=out, ld=13)
    assert np.array_equal(out[:, :10], D.snp(want)) and (out[:, 10:] == -7).all()
    out = np.full((70, 13, 5), -7, dtype=np.int32)
    synth.db_pairs(rows=(5, 70), cols=(60, 10), what=capi.PAIRS_COUNTS, out=out, ld=13)
    assert np.array_equal(out[:, :10], want) and (out[:, 10:] == -7).all()


def test_empty_ranges_succeed_and_write_nothing(synth):
    out = np.full((4, 4), -7, dtype=np.int32)
    synth.db_pairs(rows=(3, 0), cols=(0, 4), out=out)
    synth.db_pairs(rows=(130, 0), cols=(130, 0), out=out)
    synth.db_pairs(rows=(0, 4), cols=(9, 0), out=out, ld=4)
    assert (out == -7).all()
    recs, n = synth.db_pairs_within(2, rows=(3, 0), cols=(0, 4), cap=4)
    assert n == 0


# ---- word, word-group and window edges
@pytest.mark.parametrize("nchar", D.NCHARS)
def test_alignment_lengths_and_trims(nchar):
    name = "awkward9x%d" % nchar
    with loaded(name) as eng:
        for trim in D.trims_of(nchar):
            check_all(eng, D.oracle_counts(name, trim), trim=trim)


def test_trims_over_several_tiles_and_word_groups(synth):
    for trim in D.trims_of(513):
        check_all(synth, D.oracle_counts("synth130", trim), trim=trim)


def test_the_empty_window_gives_zeros():
    with loaded("awkward9x128") as eng:
        assert not eng.db_pairs(trim=64, what=capi.PAIRS_COUNTS).any()
        assert not eng.db_pairs(trim=64).any()
        recs, n = eng.db_pairs_within(0, trim=64, upper=False)
        assert n == 81 and not recs["count"].any()       # every pair is at distance 0 over no sites


# ---- content
def test_diagonal_and_symmetry(synth):
    c = synth.db_pairs(what=capi.PAIRS_COUNTS)
    assert np.array_equal(c, c.transpose(1, 0, 2))
    assert not np.diagonal(D.snp(c)).any() and not np.diagonal(D.uvaia(c)).any()
    assert D.snp(c).any() and D.uvaia(c).any()


def test_special_rows():
    with loaded("special129") as eng:
        want = D.oracle_counts("special129")
        check_all(eng, want)
        assert not want[0].any() and not want[1].any()            # all-N and all-'-' rows: nothing is compared
        assert not want[2, :, 0].any() and not want[2, :, 4].any()  # partial codes only: no ACGT site
        assert np.array_equal(want[3], want[4])                   # identical rows


def test_counters_are_wider_than_16_bits():
    nchar = 65600
    with engine(nchar, reserve=2) as eng:
        eng.db_append([b"A" * nchar, b"C" * nchar])
        assert np.array_equal(eng.db_pairs(), [[0, nchar], [nchar, 0]])
        assert np.array_equal(eng.db_pairs(what=capi.PAIRS_SNP_ALT), [[0, nchar], [nchar, 0]])
        c = eng.db_pairs(what=capi.PAIRS_COUNTS)
        assert c[0, 1].tolist() == [0, 0, 0, nchar, nchar] and c[0, 0].tolist() == [nchar] * 5
        recs, n = eng.db_pairs_within(nchar, upper=True)
        assert n == 1 and recs[0]["count"].tolist() == [0, 0, 0, nchar, nchar]


# ---- however the rows got there
def test_every_way_into_the_database_gives_the_same_matrix():
    seqs, nchar = D.case("synth130")
    want = D.oracle_counts("synth130")
    with engine(nchar) as eng:
        eng.db_append(seqs)
        check_all(eng, want)
        _planes, _non_n, side = eng.db_export()
    with engine(nchar) as eng:
        eng.db_append(seqs[:70])
        eng.db_append(seqs[70:])
        check_all(eng, want)
    with engine(nchar) as eng:
        planes, non_n = P.pack_tiles(seqs, nchar)
        eng.db_append_packed(planes, non_n, side, len(seqs))
        check_all(eng, want)
        eng.db_drop_tiles(1)
        assert eng.db_size() == 66
        check_all(eng, np.ascontiguousarray(want[64:, 64:]))


# ---- more than one launch: rows and columns beyond what one launch covers
def test_rectangles_cut_into_launches():
    n, nchar, n_rows = 8200, 33, 1030
    rng = np.random.default_rng(23)
    rows = rng.choice(np.frombuffer(b"ACGTACGTACGTNRY-", dtype=np.uint8), size=(n, nchar))
    rows[1:n_rows:5] = rows[0]                         # some pairs within a small distance
    seqs = [r.tobytes() for r in rows]
    want = D.plane_counts_of(seqs, nchar, trim=1, rows=n_rows)
    with engine(nchar, reserve=n) as eng:
        eng.db_append(seqs)
        assert np.array_equal(eng.db_pairs(rows=(0, n_rows), trim=1, what=capi.PAIRS_COUNTS), want)
        assert np.array_equal(eng.db_pairs(rows=(0, n_rows), trim=1), D.snp(want))
        expect = D.within_expected(want, 3, rows=(0, n_rows), cols=(0, n), is_rectangle=True)
        recs, found = eng.db_pairs_within(3, rows=(0, n_rows), trim=1)
        assert found == len(expect) > 1000
        assert list(zip(recs["row"].tolist(), recs["col"].tolist(), map(tuple, recs["count"].tolist()))) == expect


# ---- the list of the pairs within a distance
@pytest.mark.parametrize("metric", ["snp", "uvaia"])
@pytest.mark.parametrize("max_dist", [0, 1, 2])
def test_threshold_list(synth, max_dist, metric):
    want = D.oracle_counts("synth130")
    expect = D.within_expected(want, max_dist, metric=metric)
    if metric == "snp":
        assert len(expect) == {0: 1561, 1: 4441, 2: 6777}[max_dist]
    recs, n = synth.db_pairs_within(max_dist, metric=capi.DIST_SNP if metric == "snp" else capi.DIST_UVAIA)
    assert n == len(expect) == len(recs)
    assert list(zip(recs["row"].tolist(), recs["col"].tolist(), map(tuple, recs["count"].tolist()))) == expect


def test_threshold_without_upper_includes_the_diagonal(synth):
    want = D.oracle_counts("synth130")
    expect = D.within_expected(want, 1, upper=False, rows=(60, 10), cols=(64, 8))
    recs, n = synth.db_pairs_within(1, rows=(60, 10), cols=(64, 8), upper=False)
    assert n == len(expect)
    got = list(zip(recs["row"].tolist(), recs["col"].tolist(), map(tuple, recs["count"].tolist())))
    assert got == expect and all((i, i) in [(r, c) for r, c, _ in got] for i in range(64, 70))


@pytest.mark.parametrize("cap", [0, 1, 100])
def test_threshold_list_respects_the_capacity(synth, cap):
    sentinel = np.zeros(cap + 8, dtype=capi.PAIR_DTYPE)
    sentinel["row"], sentinel["col"], sentinel["count"] = 0xABCDEF01, 0xABCDEF02, -7
    out = sentinel.copy()
    _recs, n = synth.db_pairs_within(2, cap=cap, out=out)
    assert n == 6777
    assert np.array_equal(out[cap:], sentinel[cap:])


# ---- refusals leave the context usable
def test_refusals_leave_the_context_usable(synth):
    want = D.snp(D.oracle_counts("synth130"))
    out = np.full((140, 140), -7, dtype=np.int32)
    for kw in (dict(rows=(100, 31)), dict(cols=(131, 0)), dict(cols=(0, 131)), dict(rows=(131, 0)), dict(trim=257), dict(what=0), dict(what=4)):
        with pytest.raises(capi.GpuError) as err:
            synth.db_pairs(out=out, **{"ld": 131, **kw})
        assert err.value.code == EINVAL, kw
    for kw in (dict(max_dist=-1), dict(max_dist=1, metric=0), dict(max_dist=1, metric=3), dict(max_dist=1, trim=257), dict(max_dist=1, rows=(129, 2))):
        with pytest.raises(capi.GpuError) as err:
            synth.db_pairs_within(cap=4, **kw)
        assert err.value.code == EINVAL, kw
    with pytest.raises(capi.GpuError) as err:
        synth.db_pairs(cols=(0, 130), ld=129, out=out)
    assert err.value.code == EINVAL
    assert (out == -7).all()
    assert np.array_equal(synth.db_pairs(), want)
    assert np.array_equal(synth.db_pairs(trim=256)[:2, :2], D.snp(D.oracle_counts("synth130", 256))[:2, :2])      # 2 * trim <= nchar is fine


def test_an_acgt_context_is_refused():
    seqs, nchar = D.case("synth130")
    with engine(nchar, acgt=True) as eng:
        eng.db_append(seqs)
        with pytest.raises(capi.GpuError) as err:
            eng.db_pairs()
        assert err.value.code == ESTATE
        with pytest.raises(capi.GpuError) as err:
            eng.db_pairs_within(1)
        assert err.value.code == ESTATE
        eng.reset()
        eng.search_resident(64)                        # the context goes on working
        assert int(eng.drain()[0].sum()) > 0


# ---- non-interference
def test_a_search_sees_the_same_database_before_and_after(synth):
    def heaps():
        synth.reset()
        synth.search_resident(64)
        return [x.copy() for x in synth.drain()]
    before = heaps()
    assert int(before[0].sum()) > 0
    synth.db_pairs(what=capi.PAIRS_COUNTS)
    synth.db_pairs_within(2)
    after = heaps()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    check_all(synth, D.oracle_counts("synth130"))


def test_kernel_times_are_reported(synth):
    synth.pairs_ms(reset=True)
    synth.db_pairs()
    synth.db_pairs_within(1)
    ms = synth.pairs_ms(reset=True)
    assert ms["rows"] > 0 and ms["dense"] > 0 and ms["within"] > 0
    assert synth.pairs_ms() == {"rows": 0.0, "dense": 0.0, "within": 0.0}
