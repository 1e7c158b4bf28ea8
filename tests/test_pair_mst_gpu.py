"""uvaia_gpu_db_near_* and uvaia_gpu_db_mst against the definitions restated in pair_mst.py; every comparison is exact: the forest edge for
edge on every case, metric, trim and floor; the tree cut at D against the clusters of uvaia_gpu_db_link at D; the keys under given
components, however the matrix is cut and in whatever order; the tile pairs skipped, counted; across launches; refusals; and that nothing
else of the context is touched."""
import itertools

import numpy as np
import pytest

import pair_dist as D
import pair_edges as E
import pair_link as K
import pair_mst as M
from uvaia_amd import capi

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6
METRIC = {"snp": capi.DIST_SNP, "uvaia": capi.DIST_UVAIA}


def engine(nchar, acgt=False, reserve=256):
    eng = capi.Engine.from_query(D.dummy_query(nchar, acgt), nbest=4, max_pool=64)
    eng.db_reserve(reserve)
    return eng


def loaded_seqs(seqs, nchar):
    eng = engine(nchar, reserve=max(len(seqs), 1))
    eng.db_append(seqs)
    return eng


def loaded(name, n=None):
    seqs, nchar = M.case(name)
    return loaded_seqs(seqs[:n], nchar)


def edges_of(records):
    return [(int(a), int(b), int(d)) for a, b, d in zip(records["a"], records["b"], records["dist"])]


def floors_of(name):
    return (0, K.SYNTH_FLOOR) if name in ("synth130", "chains260x513", "dense130") else (0, 1, 5, K.SYNTH_FLOOR)


# ---- the forest, every case
@pytest.mark.parametrize("name", M.CASES)
def test_the_forest_is_kruskals(name):
    _seqs, nchar = M.case(name)
    with loaded(name) as eng:
        n = eng.db_size()
        for trim in M.trims_of(nchar):
            c = M.counts(name, trim)
            for metric in ("snp", "uvaia"):
                for floor in floors_of(name):
                    want = M.kruskal(c, metric, floor)
                    records, rounds = eng.db_mst(trim=trim, metric=METRIC[metric], min_compared=floor)
                    assert records.dtype == capi.EDGE_DTYPE and edges_of(records) == want, (trim, metric, floor)
                    assert (1 if want else 0) <= rounds <= int(np.ceil(np.log2(n))) + 1


def test_all_ties_the_hub_and_the_toy():
    with loaded("dense130") as eng:
        for metric in ("snp", "uvaia"):
            records, rounds = eng.db_mst(metric=METRIC[metric])
            assert edges_of(records) == [(0, i, 0) for i in range(1, 130)] and rounds == 1      # 8 385 edges tie at 0: the star on position 0
    with loaded("special129") as eng:
        assert edges_of(eng.db_mst()[0]) == [(0, i, 0) for i in range(1, 6)]                   # the all-N row is the hub under snp
        records, _rounds = eng.db_mst(min_compared=1)
        assert edges_of(records) == M.kruskal(M.counts("special129"), "snp", 1) and len(records) == 2 and records["a"].min() >= 3
    with loaded("toy") as eng:
        assert edges_of(eng.db_mst()[0]) == [(0, 1, 0), (0, 2, 0)]
        assert edges_of(eng.db_mst(min_compared=5)[0]) == [(0, 1, 0)]
        eng.db_near_begin(min_compared=5)
        eng.db_near()
        assert eng.db_near_fetch().tolist() == [1, 0, M.NONE]


@pytest.mark.parametrize("name", ["synth130", "chains260x513", "special129"])
def test_the_tree_cut_at_a_distance_gives_the_clusters_of_db_link(name):
    with loaded(name) as eng:
        n = eng.db_size()
        for trim, metric in itertools.product((0, 33), ("snp", "uvaia")):
            for floor in (0, K.SYNTH_FLOOR - 2 * trim if name != "special129" else 1):
                edges = edges_of(eng.db_mst(trim=trim, metric=METRIC[metric], min_compared=floor)[0])
                for max_dist in sorted({0, 1, 2, 5, max([d for _a, _b, d in edges], default=0)}):
                    eng.db_link_begin(max_dist, trim=trim, metric=METRIC[metric], min_compared=floor)
                    eng.db_link()
                    assert np.array_equal(M.components_at(n, edges, max_dist), eng.db_link_labels()), (trim, metric, floor, max_dist)


# ---- the keys under given components
def near(eng, comp=None, calls=((None, None),), **begin):
    """(keys, walked, skipped) after begin, components and one db_near per (rows, cols) of calls"""
    eng.db_near_begin(**begin)
    if comp is not None:
        eng.db_near_components(comp)
    stats = [eng.db_near(rows=r, cols=c) for r, c in calls]
    return eng.db_near_fetch(), sum(s[0] for s in stats), sum(s[1] for s in stats)


@pytest.fixture(scope="module")
def synth():
    with loaded("synth130") as eng:
        yield eng


@pytest.mark.parametrize("metric", ["snp", "uvaia"])
def test_the_keys_under_components(synth, metric):
    c = M.counts("synth130")
    n = 130
    pos = np.arange(n, dtype=np.uint32)
    first = M.nearest(c, metric)                         # a real round: everyone is united with its nearest
    one_round = K.components(n, [(x, int(first[x]) & 0xFFFFFFFF) for x in range(n)])
    assert 1 < len(set(one_round.tolist())) < n // 2
    comps = {"identity": None, "all equal": np.zeros(n, dtype=np.uint32), "// 64": pos // 64, "% 2": pos % 2, "// 32": pos // 32, "after a round": one_round}
    for floor in (0, K.SYNTH_FLOOR):
        for what, comp in comps.items():
            best, walked, skipped = near(synth, comp, metric=METRIC[metric], min_compared=floor)
            assert best.dtype == np.uint64 and np.array_equal(best, M.nearest(c, metric, floor, comp)), (what, floor)
            assert (walked, skipped) == M.tile_stats(pos if comp is None else comp, metric), (what, floor)
    best, walked, skipped = near(synth, comps["all equal"], metric=METRIC[metric])
    assert (best == M.NONE).all() and walked == 0 and skipped > 0         # every tile pair skipped, the launch itself too
    _best, walked, skipped = near(synth, comps["// 64"], metric=METRIC[metric])
    assert skipped == (130 + M.ROW_TILE[metric] - 1) // M.ROW_TILE[metric] and walked > 0       # the tile pairs on the diagonal, whole


def test_the_keys_do_not_depend_on_the_cut_or_the_order(synth):
    c = M.counts("synth130")
    n = 130
    bands = [((r, min(32, n - r)), None) for r in range(0, n, 32)]
    half = ((0, 65), (65, 65))
    quadrants = [(r, k) for r in half for k in half]      # one of them lies wholly below the diagonal
    blocks = [((r, min(48, n - r)), (k, min(40, n - k))) for r in range(0, n, 48) for k in range(0, n, 40)]
    cuts = [bands, bands[::-1], blocks, blocks[::-1], [((31, 34), None), ((0, 31), None), ((65, 65), None)]] + [list(p) for p in itertools.permutations(quadrants)][:6]
    for metric, floor, comp in (("snp", 0, None), ("snp", K.SYNTH_FLOOR, np.arange(n) % 2), ("uvaia", 0, np.arange(n) // 32)):
        want = M.nearest(c, metric, floor, comp)
        for calls in cuts:
            best, _walked, _skipped = near(synth, comp, calls=calls, metric=METRIC[metric], min_compared=floor)
            assert np.array_equal(best, want), (metric, floor, calls)
    # calls accumulate until the next components; a call below the diagonal adds nothing, and a NULL stats is fine
    synth.db_near_begin()
    assert synth.db_near(rows=(65, 65), cols=(0, 65)) == (0, 0) and (synth.db_near_fetch() == M.NONE).all()
    assert synth.db_near(rows=(0, 65), stats=False) is None
    part = synth.db_near_fetch()
    assert (part != M.NONE).all() and not np.array_equal(part, M.nearest(c, "snp"))
    synth.db_near(rows=(65, 65))
    assert np.array_equal(synth.db_near_fetch(), M.nearest(c, "snp"))
    synth.db_near_components(None)
    assert (synth.db_near_fetch() == M.NONE).all()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_database_sizes_around_a_tile(n):
    c = M.counts("synth130")[:n, :n]
    with loaded("synth130", n) as eng:
        for metric in ("snp", "uvaia"):
            best, _w, _s = near(eng, metric=METRIC[metric])
            assert np.array_equal(best, M.nearest(c, metric))
            records, rounds = eng.db_mst(metric=METRIC[metric])
            assert edges_of(records) == M.kruskal(c, metric) and len(records) == n - 1
            assert rounds == 0 if n == 1 else rounds >= 1                 # one row: no edges, zero rounds


# ---- the skip edge
@pytest.mark.parametrize("metric", ["snp", "uvaia"])
def test_one_outsider_at_the_tile_edges(metric):
    """200 rows of 129 sites, one family but one row, at lane 0 and lane 63 of a column tile, at row 0 and row 31 of a row tile, and in the
    partial last tile: the keys are exact (the outsider gets its nearest, everyone else the outsider or nothing) and exactly the tile pairs
    without it are skipped; lanes past the database neither block a skip nor fake one"""
    seqs, c = M.skip_case()
    with loaded_seqs(seqs, M.SKIP_NCHAR) as eng:
        for outsider in M.SKIP_OUTSIDERS:
            comp = M.skip_comp(outsider)
            for floor in (0, 120):
                best, walked, skipped = near(eng, comp, metric=METRIC[metric], min_compared=floor)
                assert np.array_equal(best, M.nearest(c, metric, floor, comp)), (outsider, floor)
                assert (walked, skipped) == M.tile_stats(comp, metric), (outsider, floor)
                assert skipped > walked > 0
        best, walked, skipped = near(eng, np.full(M.SKIP_N, 7, dtype=np.uint32), metric=METRIC[metric])
        assert (best == M.NONE).all() and walked == 0 and skipped == M.tile_stats(np.zeros(M.SKIP_N), metric)[1]


# ---- more than one launch
def test_across_launches():
    rows = M.launch_cut_rows()
    n = len(rows)
    assert n > M.LAUNCH_ROWS * 2
    with engine(M.LAUNCH_CUT_NCHAR, reserve=n) as eng:
        eng.db_append([r.tobytes() for r in rows])
        dist, compared = M.dist_of_bytes(rows, 1, "snp")
        edge = compared >= 0
        best, walked, skipped = near(eng, trim=1)
        assert np.array_equal(best, M.nearest_of(dist, edge)) and skipped == 0 and walked == M.tile_stats(np.arange(n), "snp")[0]
        want = M.prim_of(dist, edge)
        records, rounds = eng.db_mst(trim=1)
        assert edges_of(records) == want and len(want) == n - 1 and 1 <= rounds <= 12
        best, _w, _s = near(eng, calls=[((1024, n - 1024), None), ((0, 1024), (1000, n - 1000)), ((0, 1024), (0, 1000))], trim=1)
        assert np.array_equal(best, M.nearest_of(dist, edge))
        comp = (np.arange(n) // 1024).astype(np.uint32)                   # a band's rows and the 16 column tiles under them are one component
        best, walked, skipped = near(eng, comp, trim=1)
        assert np.array_equal(best, M.nearest_of(dist, edge, comp)) and (walked, skipped) == M.tile_stats(comp, "snp") and skipped >= 32 * 16


def test_across_launches_uvaia():
    rows = M.launch_cut_rows()[:1100]
    n = len(rows)
    with engine(M.LAUNCH_CUT_NCHAR, reserve=n) as eng:
        eng.db_append([r.tobytes() for r in rows])
        dist, compared = M.dist_of_bytes(rows, 0, "uvaia")
        edge = compared >= 129
        best, _w, _s = near(eng, metric=capi.DIST_UVAIA, min_compared=129)
        assert np.array_equal(best, M.nearest_of(dist, edge))
        records, _rounds = eng.db_mst(metric=capi.DIST_UVAIA, min_compared=129)
        assert edges_of(records) == M.prim_of(dist, edge)
        assert len(eng.db_mst(metric=capi.DIST_UVAIA, min_compared=130)[0]) == 0      # no pair is compared over more sites than there are


def test_identical_rows_at_a_size_with_more_blocks_than_cus():
    built = E.dense(E.CONTENDED_N)
    n = E.CONTENDED_N
    with engine(33, reserve=n) as eng:
        eng.db_append([r.tobytes() for r in built.rows])
        for floor in (0, 33):
            best, walked, skipped = near(eng, min_compared=floor)
            assert int(best[0]) == 1 and not best[1:].any() and skipped == 0 and walked == M.tile_stats(np.arange(n), "snp")[0]
            records, rounds = eng.db_mst(min_compared=floor)
            assert rounds == 1 and np.array_equal(records["a"], np.zeros(n - 1)) and np.array_equal(records["b"], np.arange(1, n)) and not records["dist"].any()
        records, rounds = eng.db_mst(min_compared=34)
        assert len(records) == 0 and rounds == 1                          # no edges at all: one pass finds that out


# ---- state, errors and refusals
def test_refusals_leave_the_context_usable():
    seqs, nchar = M.case("synth130")
    c = M.counts("synth130")
    with engine(nchar, reserve=140) as eng:
        eng.db_append(seqs[:100])
        for call in (eng.db_near, eng.db_near_fetch, eng.db_near_components):
            with pytest.raises(capi.GpuError) as err:      # no begin
                call()
            assert err.value.code == ESTATE
        for kw in (dict(metric=0), dict(metric=3), dict(min_compared=-1), dict(trim=257)):
            with pytest.raises(capi.GpuError) as err:
                eng.db_near_begin(**kw)
            assert err.value.code == EINVAL, kw
            with pytest.raises(capi.GpuError) as err:
                eng.db_mst(**kw)
            assert err.value.code == EINVAL, kw
        eng.db_near_begin()
        for kw in (dict(rows=(90, 11)), dict(cols=(101, 0)), dict(cols=(0, 101))):
            with pytest.raises(capi.GpuError) as err:      # a rectangle outside the database
                eng.db_near(**kw)
            assert err.value.code == EINVAL, kw
        assert eng.L.uvaia_gpu_db_near_fetch(eng.ctx, None) == EINVAL        # a NULL best
        assert eng.db_near(rows=(3, 0)) == (0, 0) and eng.db_near(cols=(9, 0)) == (0, 0)
        eng.db_near()
        assert np.array_equal(eng.db_near_fetch(), M.nearest(c[:100, :100], "snp"))
        eng.db_append(seqs[100:])
        for call in (eng.db_near, eng.db_near_fetch, eng.db_near_components):
            with pytest.raises(capi.GpuError) as err:      # the database grew since begin
                call()
            assert err.value.code == ESTATE
        assert edges_of(eng.db_mst()[0]) == M.kruskal(c, "snp")
        assert np.array_equal(near(eng, metric=capi.DIST_UVAIA, min_compared=K.SYNTH_FLOOR)[0], M.nearest(c, "uvaia", K.SYNTH_FLOOR))


def test_an_acgt_context_is_refused_and_an_empty_database_is_fine():
    seqs, nchar = M.case("synth130")
    with engine(nchar, acgt=True) as eng:
        eng.db_append(seqs)
        for call in (eng.db_near_begin, eng.db_mst, eng.db_near, eng.db_near_fetch):
            with pytest.raises(capi.GpuError) as err:
                call()
            assert err.value.code == ESTATE
        eng.reset()
        eng.search_resident(64)                        # the context goes on working
        assert int(eng.drain()[0].sum()) > 0
    with engine(nchar) as eng:
        eng.db_near_begin()
        eng.db_near_components(None)
        assert eng.db_near() == (0, 0) and eng.db_near_fetch().size == 0
        records, rounds = eng.db_mst()
        assert records.size == 0 and rounds == 0


def test_a_context_of_a_reference_shard_is_refused():
    _seqs, nchar = M.case("synth130")
    with capi.Engine.from_query(D.dummy_query(nchar), nbest=4, max_pool=256) as eng:
        eng.db_set_shard(1, 2, 128)                    # rank 1 of 2 on one card, as tests/test_refshard_gpu.py makes one
        for call in (eng.db_near_begin, eng.db_mst, eng.db_near, eng.db_near_components, eng.db_near_fetch):
            with pytest.raises(capi.GpuError) as err:
                call()
            assert err.value.code == ESTATE, call
        for kw in (dict(metric=capi.DIST_UVAIA), dict(min_compared=3), dict(trim=1)):
            with pytest.raises(capi.GpuError) as err:
                eng.db_near_begin(**kw)
            assert err.value.code == ESTATE, kw
        eng.set_active_queries(0, 2)                   # the context goes on working
        assert isinstance(eng.max_tolerance(), int)


# ---- non-interference
def test_nothing_else_of_the_context_is_touched(synth):
    def heaps():
        synth.reset()
        synth.search_resident(64)
        return [x.copy() for x in synth.drain()]
    c = M.counts("synth130")
    before = heaps()
    assert int(before[0].sum()) > 0
    synth.db_link_begin(1)
    synth.db_link()
    labels = synth.db_link_labels()
    synth.pairs_ms(reset=True)
    synth.near_ms(reset=True)
    synth.link_ms(reset=True)
    assert edges_of(synth.db_mst(min_compared=K.SYNTH_FLOOR)[0]) == M.kruskal(c, "snp", K.SYNTH_FLOOR)
    assert edges_of(synth.db_mst(metric=capi.DIST_UVAIA)[0]) == M.kruskal(c, "uvaia")
    ms = synth.pairs_ms()
    assert synth.near_ms(reset=True) > 0 and synth.near_ms() == 0 and ms["rows"] > 0 and ms["dense"] == 0 and ms["within"] == 0 and synth.link_ms() == 0
    assert np.array_equal(synth.db_link_labels(), labels) and np.array_equal(labels, K.restate(c, "snp", 1)[0])      # the forest of db_link is still open
    after = heaps()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(synth.db_pairs(what=capi.PAIRS_COUNTS), c)
    assert synth.db_pairs_within(1, cap=0)[1] == K.restate(c, "snp", 1)[1] == synth.db_link()
