"""uvaia_gpu_db_link_begin / _link / _link_labels against the definition restated in pair_link.py: the label of every row and the number
of links, exactly, for every case, metric, distance and floor; at the tile, word and window edges; however the matrix is cut and in
whatever order; across launches; refusals; and that a search before and after sees the same database."""
import itertools

import numpy as np
import pytest

import pair_dist as D
import pair_link as K
from uvaia_amd import capi

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6
METRIC = {"snp": capi.DIST_SNP, "uvaia": capi.DIST_UVAIA}


def engine(nchar, acgt=False, reserve=256):
    eng = capi.Engine.from_query(D.dummy_query(nchar, acgt), nbest=4, max_pool=64)
    eng.db_reserve(reserve)
    return eng


def loaded(name, n=None):
    seqs, nchar = K.case(name)
    seqs = seqs[:n]
    eng = engine(nchar, reserve=len(seqs))
    eng.db_append(seqs)
    return eng


def cluster(eng, max_dist, metric="snp", floor=0, trim=0, calls=((None, None),)):
    """(labels, links) after begin and one db_link per (rows, cols) of calls"""
    eng.db_link_begin(max_dist, trim=trim, metric=METRIC[metric], min_compared=floor)
    links = sum(eng.db_link(rows=r, cols=c) for r, c in calls)
    return eng.db_link_labels(), links


def check(eng, counts, max_dist, metric, floor, trim=0):
    want, n_want = K.restate(counts, metric, max_dist, floor)
    got, n_got = cluster(eng, max_dist, metric, floor, trim)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (metric, max_dist, floor, trim, np.flatnonzero(got != want)[:8].tolist())
    assert n_got == n_want, (metric, max_dist, floor, trim)
    if floor == 0:
        _recs, n_within = eng.db_pairs_within(max_dist, trim=trim, metric=METRIC[metric], upper=True, cap=0)
        assert n_got == n_within


# ---- every case, metric, distance, with the floor off and on
@pytest.fixture(scope="module")
def chains():
    with loaded("chains260x513") as eng:
        yield eng


@pytest.fixture(scope="module")
def synth():
    with loaded("synth130") as eng:
        yield eng


@pytest.mark.parametrize("metric", ["snp", "uvaia"])
def test_chains(chains, metric):
    c = K.counts("chains260x513")
    for max_dist in (0, 1, 2):
        for floor in (0, 513, 514):                   # every pair is compared over 513 sites: the floor is met, then missed by one
            check(chains, c, max_dist, metric, floor)
    labels, links = cluster(chains, 1, metric)
    assert sorted(np.bincount(labels)[np.unique(labels)].tolist()) == sorted(K.CHAIN_FAMILIES) and links == 252
    labels, links = cluster(chains, 0, metric)
    assert np.array_equal(labels, np.arange(260)) and links == 0
    labels, links = cluster(chains, 1, metric, floor=514)
    assert np.array_equal(labels, np.arange(260)) and links == 0


@pytest.mark.parametrize("metric", ["snp", "uvaia"])
def test_dense_rows_are_one_cluster(metric):
    with loaded("dense130") as eng:
        for floor in (0, 513):
            labels, links = cluster(eng, 0, metric, floor)
            assert not labels.any() and links == 130 * 129 // 2
            check(eng, K.counts("dense130"), 0, metric, floor)


def test_special_rows_and_the_floor():
    with loaded("special129") as eng:
        c = K.counts("special129")
        for metric in ("snp", "uvaia"):
            for max_dist in (0, 1):
                for floor in (0, 1, 129, 130):
                    check(eng, c, max_dist, metric, floor)
        labels, _links = cluster(eng, 0, "snp", floor=0)
        assert not labels.any()                       # an all-N row is at distance 0 from every row: the definition
        labels, _links = cluster(eng, 0, "snp", floor=1)
        assert labels.tolist() == [0, 1, 2, 3, 3, 5]


@pytest.mark.parametrize("metric", ["snp", "uvaia"])
@pytest.mark.parametrize("max_dist", [0, 1, 2])
def test_synth130(synth, max_dist, metric):
    c = K.counts("synth130")
    for floor in (0, 1, K.SYNTH_FLOOR):
        check(synth, c, max_dist, metric, floor)


# ---- lane and tile edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_database_sizes_around_a_tile(n):
    c = K.counts("synth130")[:n, :n]
    with loaded("synth130", n) as eng:
        for metric in ("snp", "uvaia"):
            for floor in (0, K.SYNTH_FLOOR):
                check(eng, c, 1, metric, floor)


# ---- word, word-group and window edges
@pytest.mark.parametrize("nchar", D.NCHARS)
def test_alignment_lengths_and_trims(nchar):
    name = "awkward9x%d" % nchar
    with loaded(name) as eng:
        for trim in D.trims_of(nchar):
            c = D.oracle_counts(name, trim)
            some = sorted(set(np.percentile(D.snp(c), (0, 25, 50)).astype(int).tolist()))      # distances at which some pairs link and some do not
            floor = int(np.median(c[..., 4]))
            for metric in ("snp", "uvaia"):
                for max_dist in some:
                    check(eng, c, max_dist, metric, 0, trim)
                    check(eng, c, max_dist, metric, max(floor, 1), trim)


def test_the_empty_window():
    with loaded("awkward9x128") as eng:
        for metric in ("snp", "uvaia"):
            labels, links = cluster(eng, 0, metric, floor=0, trim=64)       # every distance is 0 over no sites
            assert not labels.any() and links == 36
            labels, links = cluster(eng, 0, metric, floor=1, trim=64)       # ... and nothing was compared
            assert np.array_equal(labels, np.arange(9)) and links == 0


# ---- the answer does not depend on how the matrix is cut, nor on the order
def test_order_independence(chains):
    c = K.counts("chains260x513")
    want, n_want = K.restate(c, "snp", 1)
    bands = [((r, min(64, 260 - r)), None) for r in range(0, 260, 64)]
    half = ((0, 130), (130, 130))
    quadrants = [(r, k) for r in half for k in half]
    cuts = [[(None, None)], bands[::-1], [((31, 34), (0, 260)), ((0, 31), None), ((65, 195), None)]]
    cuts += [list(p) for p in itertools.permutations(quadrants)]
    for metric, floor in (("snp", 0), ("snp", 513), ("uvaia", 0)):
        for calls in cuts:
            labels, links = cluster(chains, 1, metric, floor, calls=calls)
            assert np.array_equal(labels, want) and links == n_want, (metric, floor, calls)
    # the same rectangle twice: its links are counted twice, the clusters do not change
    part, n_part = K.restate(c, "snp", 1, rows=(31, 34))
    labels, links = cluster(chains, 1, calls=[((31, 34), (0, 260))] * 2)
    assert np.array_equal(labels, part) and links == 2 * n_part > 0


def test_a_rectangle_below_the_diagonal_has_no_links(chains):
    chains.db_link_begin(1)
    assert chains.db_link(rows=(130, 130), cols=(130, 130)) > 0
    for _ in range(3):                                # nothing is launched: the count is 0, not what the call before left
        assert chains.db_link(rows=(130, 130), cols=(0, 130)) == 0
        assert chains.db_link(rows=(64, 1), cols=(0, 65)) == 0
    assert chains.db_link(rows=(64, 1), cols=(0, 66)) == int(K.linked(K.counts("chains260x513"), "snp", 1)[64, 65])


def test_labels_between_links_show_the_partial_components(chains):
    c = K.counts("chains260x513")
    chains.db_link_begin(1)
    assert np.array_equal(chains.db_link_labels(), np.arange(260))
    done = 0
    for r in range(0, 260, 64):
        done += chains.db_link(rows=(r, min(64, 260 - r)))
        want, n_want = K.restate(c, "snp", 1, rows=(0, min(r + 64, 260)))
        assert np.array_equal(chains.db_link_labels(), want) and done == n_want
        assert np.array_equal(chains.db_link_labels(), want)      # reading the labels changes nothing
    assert np.array_equal(chains.db_link_labels(), K.restate(c, "snp", 1)[0])


# ---- more than one launch: rows and columns beyond what one launch covers
def test_links_across_launches():
    n, nchar = 8200, 33
    rng = np.random.default_rng(23)
    rows = rng.choice(np.frombuffer(b"ACGTACGTACGTNRY-", dtype=np.uint8), size=(n, nchar))
    rows[1:1030:5] = rows[0]                           # a dense cluster inside the first launch's rows
    family = (5, 1023, 1024, 1025, 8191, 8192, 8199)   # a chain over the edges of the 1 024-row and 8 192-column launches
    base = bytearray(np.random.default_rng(41).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nchar).tobytes())
    for k, pos in enumerate(family):
        rows[pos] = np.frombuffer(bytes(base), dtype=np.uint8)
        base[2 + 4 * k] = b"ACGT"[(b"ACGT".index(base[2 + 4 * k]) + 1) % 4]
    pairs = K.snp_links_of_bytes(rows, 1, 1)
    want = K.components(n, pairs)
    assert all(want[p] == 5 for p in family) and int((want == 5).sum()) == len(family)
    assert all([a, b] in pairs.tolist() for a, b in zip(family, family[1:])) and [5, 1024] not in pairs.tolist()
    assert int((want == 0).sum()) >= 207
    with engine(nchar, reserve=n) as eng:
        eng.db_append([r.tobytes() for r in rows])
        labels, links = cluster(eng, 1, trim=1)
        assert np.array_equal(labels, want) and links == len(pairs)
        labels, links = cluster(eng, 1, trim=1, floor=1)
        assert np.array_equal(labels, want) and links == len(pairs)          # (a linked pair here has compared sites)
        labels, links = cluster(eng, 1, trim=1, calls=[((1024, 7176), None), ((0, 1024), None)])
        assert np.array_equal(labels, want) and links == len(pairs)


# ---- refusals leave the context usable
def test_refusals_leave_the_context_usable():
    seqs, nchar = K.case("synth130")
    c = K.counts("synth130")
    with engine(nchar, reserve=140) as eng:
        eng.db_append(seqs[:100])
        for call in (eng.db_link, eng.db_link_labels):
            with pytest.raises(capi.GpuError) as err:      # no begin
                call()
            assert err.value.code == ESTATE
        for kw in (dict(max_dist=-1), dict(max_dist=1, metric=0), dict(max_dist=1, metric=3), dict(max_dist=1, min_compared=-1), dict(max_dist=1, trim=257)):
            with pytest.raises(capi.GpuError) as err:
                eng.db_link_begin(**kw)
            assert err.value.code == EINVAL, kw
        eng.db_link_begin(1)
        for kw in (dict(rows=(90, 11)), dict(cols=(101, 0)), dict(cols=(0, 101))):
            with pytest.raises(capi.GpuError) as err:      # a rectangle outside the database
                eng.db_link(**kw)
            assert err.value.code == EINVAL, kw
        assert eng.db_link(rows=(3, 0)) == 0 and eng.db_link(cols=(9, 0)) == 0
        assert eng.db_link() == K.restate(c[:100, :100], "snp", 1)[1]
        assert np.array_equal(eng.db_link_labels(), K.restate(c[:100, :100], "snp", 1)[0])
        eng.db_append(seqs[100:])
        for call in (eng.db_link, eng.db_link_labels):
            with pytest.raises(capi.GpuError) as err:      # the database grew since begin
                call()
            assert err.value.code == ESTATE
        check(eng, c, 1, "snp", 0)
        check(eng, c, 2, "uvaia", K.SYNTH_FLOOR)


def test_an_acgt_context_is_refused():
    seqs, nchar = K.case("synth130")
    with engine(nchar, acgt=True) as eng:
        eng.db_append(seqs)
        for call in (lambda: eng.db_link_begin(1), eng.db_link, eng.db_link_labels):
            with pytest.raises(capi.GpuError) as err:
                call()
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
    c = K.counts("synth130")
    check(synth, c, 2, "snp", K.SYNTH_FLOOR)
    check(synth, c, 2, "uvaia", 0)
    after = heaps()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(synth.db_pairs(what=capi.PAIRS_COUNTS), c)
    assert np.array_equal(synth.db_link_labels(), K.restate(c, "uvaia", 2)[0])      # the clustering is still open behind a search


def test_kernel_time_has_a_slot_of_its_own(synth):
    synth.pairs_ms(reset=True)
    synth.link_ms(reset=True)
    cluster(synth, 1)
    ms = synth.pairs_ms()
    assert synth.link_ms(reset=True) > 0 and ms["rows"] > 0 and ms["dense"] == 0 and ms["within"] == 0
    assert synth.link_ms() == 0
