"""The all-pairs kernels at the edges their feature tests leave out (tests/pair_edges.py has the inputs and the restatements):
  A  the forest of uvaia_gpu_db_link under contention: one launch with more blocks than the chip has CUs, all hooking into the same few
     roots -- identical rows, a chain as deep as the component, a hub at the smallest and at the largest position, two dense halves and a
     bridge -- labels and link counts exactly, however the matrix is cut;
  B  tiles that were handed in with stale lanes past the last row and stale bits at and past nchar: every pair entry as over clean tiles;
  C  the launch cut for the forms that never crossed it: the uvaia link kernel, the ALT snp tile, columns that begin mid-tile, a skipped
     launch and a capacity that runs out in the list form;
  D  word-group counts 3, 4 and 8, one and two sites, thresholds above 16 bits and at INT_MAX, an empty and a replaced database.
Expected values come from the construction, pair_dist.plane_counts_of / oracle_counts, pair_link.components / restate /
snp_links_of_bytes and pair_edges.uvaia_links_of_bytes (pinned to the plane counters in test_pair_edges_cpu.py), never from an engine."""
import numpy as np
import pytest

import pair_dist as D
import pair_edges as E
import pair_link as K
from uvaia_amd import capi

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6
METRIC = {"snp": capi.DIST_SNP, "uvaia": capi.DIST_UVAIA}
N, NCHAR = E.CONTENDED_N, E.CONTENDED_NCHAR


def engine(nchar, reserve=256):
    eng = capi.Engine.from_query(D.dummy_query(nchar) if nchar >= 5 else E.short_query(nchar), nbest=4, max_pool=64)
    eng.db_reserve(reserve)
    return eng


def loaded_rows(rows):
    eng = engine(rows.shape[1], reserve=len(rows))
    eng.db_append_block(rows)
    return eng


def cluster(eng, max_dist, metric="snp", floor=0, trim=0, calls=((None, None),)):
    """(labels, links) after begin and one db_link per (rows, cols) of calls"""
    eng.db_link_begin(max_dist, trim=trim, metric=METRIC[metric], min_compared=floor)
    links = sum(eng.db_link(rows=r, cols=c) for r, c in calls)
    return eng.db_link_labels(), links


def expect(eng, want, n_want, max_dist, metric="snp", floor=0, trim=0, calls=((None, None),), note=None):
    got, n_got = cluster(eng, max_dist, metric, floor, trim, calls)
    note = (note, metric, max_dist, floor, trim, len(calls))
    assert got.dtype == np.uint32 and np.array_equal(got, want), (note, np.flatnonzero(got != want)[:8].tolist(), got[got != want][:8].tolist())
    assert n_got == n_want, note


def records(recs):
    return list(zip(recs["row"].tolist(), recs["col"].tolist(), map(tuple, recs["count"].tolist())))


# ------------------------------------------------------------------------------------------------------------------ A: contention
def test_dense_rows_in_one_launch():
    built = E.dense(N)
    identity = np.arange(N, dtype=np.uint32)
    with loaded_rows(built.rows) as eng:
        for calls in ([(None, None)], E.bands_reversed(N)):
            for metric, floor in (("snp", 0), ("snp", 33), ("uvaia", 0), ("uvaia", 33)):
                expect(eng, built.labels[0], built.links[0], 0, metric, floor, calls=calls, note="dense")
            expect(eng, identity, 0, 0, "snp", 34, calls=calls, note="dense, floor missed by one")
            expect(eng, identity, 0, 0, "uvaia", 34, calls=calls, note="dense, floor missed by one")


@pytest.mark.parametrize("order", E.POSITION_MAPS)
def test_chain(order):
    built = E.chain(N, NCHAR, order)
    pairs = E.construction_links(built, 1)
    with loaded_rows(built.rows) as eng:
        for metric in ("snp", "uvaia"):
            expect(eng, built.labels[1], N - 1, 1, metric, note=order)
            expect(eng, built.labels[0], 0, 0, metric, note=order)
        expect(eng, built.labels[1], N - 1, 1, "uvaia", calls=E.bands_reversed(N), note=order)
        # bands of 64 rows, last band first, the labels read after every band: the components of the pairs of the bands done so far
        eng.db_link_begin(1)
        done, links = np.zeros(len(pairs), dtype=bool), 0
        for (r0, nr), cols in E.bands_reversed(N):
            links += eng.db_link(rows=(r0, nr), cols=cols)
            done |= (pairs[:, 0] >= r0) & (pairs[:, 0] < r0 + nr)
            assert links == int(done.sum()), (order, r0)
            got = eng.db_link_labels()
            assert np.array_equal(got, K.components(N, pairs[done])), (order, r0)
        assert done.all() and np.array_equal(got, built.labels[1])
        if order == "identity":                      # the same rectangle twice: the clusters do not change, the links are counted twice
            inside = (pairs[:, 0] >= 31) & (pairs[:, 0] < 3031)
            expect(eng, K.components(N, pairs[inside]), 2 * int(inside.sum()), 1, calls=[((31, 3000), None)] * 2, note="twice")


@pytest.mark.parametrize("hub_at", [0, N - 1])
def test_star(hub_at):
    built = E.star(N, NCHAR, hub_at)
    with loaded_rows(built.rows) as eng:
        for metric in ("snp", "uvaia"):
            for calls in ([(None, None)], E.bands_reversed(N)):
                expect(eng, built.labels[1], N - 1, 1, metric, calls=calls, note=hub_at)
            expect(eng, built.labels[0], 0, 0, metric, note=hub_at)


def test_two_dense_halves_and_a_bridge():
    built = E.bridged(N)
    assert sorted(set(built.labels[0].tolist())) == [0, 1, N - 1]
    with loaded_rows(built.rows) as eng:
        for metric in ("snp", "uvaia"):
            for calls in ([(None, None)], E.bands_reversed(N), E.quadrants(N), E.quadrants(N)[::-1]):
                for max_dist in (0, 1):
                    expect(eng, built.labels[max_dist], built.links[max_dist], max_dist, metric, calls=calls, note="bridged")
                expect(eng, built.labels[1], built.links[1], 1, metric, 33, calls=calls, note="bridged, floor met")


# ------------------------------------------------------------------------------------------------------------------ B: stale bits
def check_counts(eng, want, trim, rows=None, cols=None):
    """the counters and both snp tiles of a rectangle against want[rows, cols]"""
    n = want.shape[0]
    r0, nr = rows or (0, n)
    c0, nc = cols or (0, n)
    w = want[r0:r0 + nr, c0:c0 + nc]
    got = eng.db_pairs(rows=(r0, nr), cols=(c0, nc), trim=trim, what=capi.PAIRS_COUNTS)
    bad = np.argwhere(got != w)
    assert got.shape == w.shape and bad.size == 0, "counters differ at (row, col, counter) %r ... got %r want %r" % (bad[:5].tolist(), got[tuple(bad[0])], w[tuple(bad[0])])
    for what in (capi.PAIRS_SNP, capi.PAIRS_SNP_ALT):
        assert np.array_equal(eng.db_pairs(rows=(r0, nr), cols=(c0, nc), trim=trim, what=what), D.snp(w)), what


def check_every_pair_entry(eng, want, trim, note):
    """db_pairs with all three outputs, db_pairs_within under both metrics, and the clusters (snp floor off and on, uvaia), whole and
    over a rectangle that is not tile-aligned, against the counters `want` of every pair"""
    rect = dict(rows=(5, 70), cols=(60, 68))
    check_counts(eng, want, trim)
    check_counts(eng, want, trim, **rect)
    for metric in ("snp", "uvaia"):
        dist, compared = (D.snp(want), want[..., 4]) if metric == "snp" else (D.uvaia(want), want[..., 3])
        floor = max(int(np.median(compared)), 1)
        for max_dist in sorted(set(np.percentile(dist, (25, 50)).astype(int).tolist())):      # some pairs within it and some not
            for kw in (dict(), rect):
                recs, n = eng.db_pairs_within(max_dist, trim=trim, metric=METRIC[metric], **kw)
                assert records(recs) == D.within_expected(want, max_dist, metric=metric, **kw) and n == len(recs), (note, metric, kw)
            for fl in (0, floor):
                labels, links = K.restate(want, metric, max_dist, fl)
                expect(eng, labels, links, max_dist, metric, fl, trim, note=note)
                labels, links = K.restate(want, metric, max_dist, fl, **rect)
                expect(eng, labels, links, max_dist, metric, fl, trim, calls=[(rect["rows"], rect["cols"])], note=note)


@pytest.mark.parametrize("name", ["awkward130x129", "synth130"])
def test_stale_lanes_and_bits_in_handed_in_tiles_never_count(name):
    """the comment above pairs_rows_kernel: sites at and past nchar never count, "zero in tiles this library packed, anything in tiles
    that were handed in", and the column side needs no mask.  non_n and the side rows stay clean; only the pair entries are called."""
    seqs, nchar = D.case(name)
    n = len(seqs)
    with engine(nchar, reserve=n) as eng:
        eng.db_append(seqs)
        planes, non_n, side = eng.db_export()
    wants = [(trim, D.oracle_counts(name, trim)) for trim in (0, 1, nchar // 2)]
    for how in (None, "lanes", "bits", "both"):
        tiles = planes if how is None else E.dirty(planes, n, nchar, how)
        assert (how is None) == np.array_equal(tiles, planes)
        with engine(nchar, reserve=n) as eng:
            eng.db_append_packed(tiles, non_n, side, n)
            for trim, want in wants:
                check_every_pair_entry(eng, want, trim, (name, how, trim))


# ------------------------------------------------------------------------------------------------------------------ C: the launch cut
T = E.LAUNCH_TRIM


@pytest.fixture(scope="module")
def launches():
    with loaded_rows(E.launch_rows()) as eng:
        yield eng


def test_uvaia_links_across_launches(launches):
    """pairs_counts_kernel<PAIRS_LINK> takes `row0 + rb` in the `row < col` test and in the forest index.  Two references: the calls over
    the bands (0, 1 030) and (8 185, 15) -- both launch edges, every link of the chain family -- are judged by the plane counters of
    exactly those rows; the whole matrix and its cut at row 1 024 by pair_edges.uvaia_links_of_bytes over all pairs, which
    test_pair_edges_cpu.py pins to the plane counters on those bands."""
    n = E.LAUNCH_N
    bands = ((0, 1030), (8185, 15))
    for floor in (0, E.launch_floor()):
        pairs = np.concatenate([E.band_links(E.launch_counts(*b), b[0], "uvaia", 1, floor) for b in bands])
        assert set(zip(E.LAUNCH_FAMILY, E.LAUNCH_FAMILY[1:])) <= set(map(tuple, pairs.tolist()))
        expect(launches, K.components(n, pairs), len(pairs), 1, "uvaia", floor, T, calls=[(b, None) for b in bands], note="bands")
        pairs = E.launch_links("uvaia", 1, floor)
        want = K.components(n, pairs)
        for calls in ([(None, None)], [((1024, 7176), None), ((0, 1024), None)]):
            expect(launches, want, len(pairs), 1, "uvaia", floor, T, calls=calls, note="all pairs")


def test_the_alt_tile_across_launches(launches):
    want = D.snp(E.launch_counts(0, 1030))
    got = launches.db_pairs(rows=(0, 1030), trim=T, what=capi.PAIRS_SNP_ALT)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


@pytest.mark.parametrize("cols", [(63, 8137), (5, 8195)])
def test_columns_that_begin_mid_tile(launches, cols):
    """(63, 8 137): one launch of 8 137 columns from lane 63 of tile 0 to the last row.  (5, 8 195): two launches, the second begins at
    column 8 197, inside tile 128, and covers three columns."""
    rows = (1000, 60)
    want = E.launch_counts(*rows)[:, cols[0]:cols[0] + cols[1]]
    assert (cols[1] > E.LAUNCH_COLS) == (cols == (5, 8195)) and cols[0] % 64 and cols[0] + cols[1] == E.LAUNCH_N
    got = launches.db_pairs(rows=rows, cols=cols, trim=T, what=capi.PAIRS_COUNTS)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    for what in (capi.PAIRS_SNP, capi.PAIRS_SNP_ALT):
        assert np.array_equal(launches.db_pairs(rows=rows, cols=cols, trim=T, what=what), D.snp(want)), what
    for metric, max_dist in (("snp", 3), ("uvaia", 6)):
        for upper in (True, False):
            expected = D.within_expected(want, max_dist, metric=metric, upper=upper, rows=rows, cols=cols, is_rectangle=True)
            recs, found = launches.db_pairs_within(max_dist, rows=rows, cols=cols, trim=T, metric=METRIC[metric], upper=upper)
            assert found == len(expected) > 0 and records(recs) == expected, (metric, upper)
    pairs = E.band_links(E.launch_counts(*rows), rows[0], "snp", 3, cols=cols)
    expect(launches, K.components(E.LAUNCH_N, pairs), len(pairs), 3, trim=T, calls=[(rows, cols)], note="mid-tile")
    assert len(pairs) > 0


def test_a_skipped_launch_in_the_list_form(launches):
    """rows (8 192, 8) with upper: the first column launch (columns 0 .. 8 191) lies at or below the diagonal and is skipped; without
    upper it runs.  rows (1 020, 10): nothing is skipped, the first launch holds the rows' own diagonal."""
    n = E.LAUNCH_N
    for rows, counts in (((8192, 8), E.launch_counts(8192, 8)), ((1020, 10), E.launch_counts(0, 1030)[1020:1030])):
        for metric, max_dist in (("snp", 3), ("uvaia", 6)):
            for upper in (True, False):
                expected = D.within_expected(counts, max_dist, metric=metric, upper=upper, rows=rows, cols=(0, n), is_rectangle=True)
                recs, found = launches.db_pairs_within(max_dist, rows=rows, trim=T, metric=METRIC[metric], upper=upper)
                assert found == len(expected) > 0 and records(recs) == expected, (rows, metric, upper)
                _recs, found = launches.db_pairs_within(max_dist, rows=rows, trim=T, metric=METRIC[metric], upper=upper, cap=0)
                assert found == len(expected)
    assert (8192, 8199) in [(r, c) for r, c, _k in D.within_expected(E.launch_counts(8192, 8), 3, rows=(8192, 8), cols=(0, n), is_rectangle=True)]


def test_the_capacity_runs_out_in_a_later_launch(launches):
    """rows (1 020, 10) against all columns are two launches (columns 0 .. 8 191 and 8 192 .. 8 199): `room = cap - found`, the copy to
    `out + found`.  n_found is the number of hits whatever fitted, the slots at and past cap are not written, the slots below it hold
    distinct genuine hits, and a list that fits is the sorted expected list."""
    rows, n, max_dist = (1020, 10), E.LAUNCH_N, 3
    counts = E.launch_counts(0, 1030)[1020:1030]
    expected = D.within_expected(counts, max_dist, rows=rows, cols=(0, n), is_rectangle=True)
    f1 = sum(1 for _r, c, _k in expected if c < E.LAUNCH_COLS)
    f2 = len(expected) - f1
    assert f1 > 1 and f2 > 1
    for cap in (f1 - 1, f1, f1 + 1, f1 + f2 - 1, f1 + f2):
        sentinel = np.zeros(f1 + f2 + 8, dtype=capi.PAIR_DTYPE)
        sentinel["row"], sentinel["col"], sentinel["count"] = 0xABCDEF01, 0xABCDEF02, -7
        out = sentinel.copy()
        _recs, found = launches.db_pairs_within(max_dist, rows=rows, trim=T, cap=cap, out=out)
        assert found == f1 + f2, cap
        assert np.array_equal(out[cap:], sentinel[cap:]), cap
        got = records(out[:min(cap, found)])
        assert len(set(got)) == len(got) and set(got) <= set(expected), cap
        if cap == f1 + f2:
            assert got == expected


# ------------------------------------------------------------------------------------------------------------------ D: shapes and widths
@pytest.mark.parametrize("nchar", [1, 2, 257, 384, 385, 512, 1024])          # W4 = 1, 1, 3, 3, 4, 4, 8
def test_more_alignment_lengths(nchar):
    name = "awkward9x%d" % nchar
    seqs, _nchar = D.case(name)
    assert ((nchar + 31) // 32 + 3) // 4 == {1: 1, 2: 1, 257: 3, 384: 3, 385: 4, 512: 4, 1024: 8}[nchar]
    with engine(nchar, reserve=len(seqs)) as eng:
        eng.db_append(seqs)
        for trim in D.trims_of(nchar):
            c = D.oracle_counts(name, trim)
            check_counts(eng, c, trim)
            some = sorted(set(np.percentile(D.snp(c), (0, 25, 50)).astype(int).tolist()))
            floor = max(int(np.median(c[..., 4])), 1)
            for metric in ("snp", "uvaia"):
                for max_dist in some:
                    for upper in (True, False):
                        recs, found = eng.db_pairs_within(max_dist, trim=trim, metric=METRIC[metric], upper=upper)
                        assert records(recs) == D.within_expected(c, max_dist, metric=metric, upper=upper) and found == len(recs), (trim, metric, max_dist)
                    for fl in (0, floor):
                        labels, links = K.restate(c, metric, max_dist, fl)
                        expect(eng, labels, links, max_dist, metric, fl, trim, note=nchar)


@pytest.mark.parametrize("metric", ["snp", "uvaia"])
def test_thresholds_above_16_bits_and_at_int_max(metric):
    nchar = 65600
    apart, together = np.array([0, 1], dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    with engine(nchar, reserve=2) as eng:
        eng.db_append([b"A" * nchar, b"C" * nchar])                  # distance 65 600 over 65 600 compared sites under both metrics
        expect(eng, together, 1, nchar, metric)
        expect(eng, apart, 0, nchar - 1, metric)
        expect(eng, together, 1, nchar, metric, floor=nchar)
        expect(eng, apart, 0, nchar, metric, floor=nchar + 1)
        expect(eng, together, 1, D.INT_MAX, metric)
        expect(eng, together, 1, D.INT_MAX, metric, floor=nchar)
        expect(eng, apart, 0, D.INT_MAX, metric, floor=D.INT_MAX)
        expect(eng, together, 1, nchar - 2, metric, trim=1)         # 65 598 sites in the window
        expect(eng, apart, 0, nchar - 3, metric, trim=1)
        for max_dist, n_want in ((nchar, 1), (nchar - 1, 0), (D.INT_MAX, 1)):
            recs, found = eng.db_pairs_within(max_dist, metric=METRIC[metric])
            assert found == n_want and [(r, c) for r, c, _k in records(recs)] == [(0, 1)] * n_want


def test_an_empty_database():
    with engine(33, reserve=64) as eng:
        assert eng.db_size() == 0
        for metric in ("snp", "uvaia"):
            eng.db_link_begin(1, metric=METRIC[metric], min_compared=1)
            assert eng.db_link() == 0
            assert eng.db_link_labels().shape == (0,)
            recs, found = eng.db_pairs_within(1, metric=METRIC[metric])
            assert found == 0 and len(recs) == 0
        for what in (capi.PAIRS_SNP, capi.PAIRS_SNP_ALT, capi.PAIRS_COUNTS):
            assert eng.db_pairs(what=what).size == 0
        seqs = D.case("awkward9x33")[0]                              # the context goes on working
        eng.db_append(seqs)
        check_counts(eng, D.oracle_counts("awkward9x33"), 0)


def test_a_database_replaced_after_begin():
    """link_state rests on the database generation: the same number of rows after a clear, or after dropped tiles and a refill, is
    another database, and the forest of the old one is refused"""
    seqs, nchar = K.case("synth130")
    c = K.counts("synth130")
    want, n_want = K.restate(c, "snp", 1)

    def refused():
        for call in (eng.db_link, eng.db_link_labels):
            with pytest.raises(capi.GpuError) as err:
                call()
            assert err.value.code == ESTATE
    with engine(nchar, reserve=192) as eng:
        eng.db_append(seqs)
        eng.db_link_begin(1)
        assert eng.db_link(rows=(0, 64)) > 0
        eng.db_clear()
        refused()
        eng.db_append(seqs)                                          # the same rows, the same size
        assert eng.db_size() == 130
        refused()
        expect(eng, want, n_want, 1)
        eng.db_drop_tiles(1)                                         # 66 rows left ...
        refused()
        eng.db_append(seqs[:64])                                     # ... and 130 again: rows 64 .. 129, then rows 0 .. 63
        assert eng.db_size() == 130
        refused()
        order = list(range(64, 130)) + list(range(64))
        moved = np.ascontiguousarray(c[order][:, order])
        for metric, floor in (("snp", 0), ("uvaia", K.SYNTH_FLOOR)):
            labels, links = K.restate(moved, metric, 1, floor)
            expect(eng, labels, links, 1, metric, floor)
