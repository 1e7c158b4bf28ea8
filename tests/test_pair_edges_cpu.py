"""The inputs of tests/pair_edges.py without a GPU: the builders have the distances, links and clusters their GPU tests take from the
construction; the matrix-product restatement of the uvaia links equals the plane counters; the dirtied tiles keep every bit that counts;
and the argument of DESIGN.md 4.12 -- stale loads cost time, never the answer -- holds in a step-by-step model of the forest, which
does see a lost hook once the compare-and-swap is taken apart."""
import numpy as np
import pytest

import fixtures as F
import oracle_lib as O
import packed_lib as P
import pair_dist as D
import pair_edges as E
import pair_link as K


def small_cases():
    n = E.SMALL_N
    nchar = n + 4
    out = [("dense", E.dense(n)), ("bridged", E.bridged(n))]
    out += [("chain-" + m, E.chain(n, nchar, m)) for m in ("identity", "reversed")]
    out += [("chain-mod77", E.chain(n + 1, nchar, "mod77"))]          # 77 does not divide 261
    out += [("star-hub%d" % h, E.star(n, nchar, h)) for h in (0, n - 1)]
    return out


def contended_cases():
    n, nchar = E.CONTENDED_N, E.CONTENDED_NCHAR
    out = [("chain-" + m, E.chain(n, nchar, m)) for m in E.POSITION_MAPS]
    out += [("star-hub%d" % h, E.star(n, nchar, h)) for h in (0, n - 1)]
    return out


def byte_distances(rows, p):
    return (rows != rows[p]).sum(axis=1)


# ---- A: the builders
@pytest.mark.parametrize("name, built", small_cases(), ids=[c[0] for c in small_cases()])
def test_every_pair_of_a_small_builder(name, built):
    rows = built.rows
    n = len(rows)
    assert np.isin(rows, np.frombuffer(b"ACGT", dtype=np.uint8)).all()
    dist = (rows[:, None, :] != rows[None, :, :]).sum(axis=2)                          # ACGT everywhere: the snp distance is the byte distance
    for p in range(n):
        assert np.array_equal(dist[p], E.distances_from(built, p)), (name, p)
    upper = np.arange(n)[:, None] < np.arange(n)[None, :]
    for max_dist in (0, 1):
        pairs = np.argwhere((dist <= max_dist) & upper)
        got = K.snp_links_of_bytes(rows, 0, max_dist, block=64)
        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, pairs.tolist())), (name, max_dist)
        assert len(pairs) == built.links[max_dist], (name, max_dist)
        assert np.array_equal(K.components(n, pairs), built.labels[max_dist]), (name, max_dist)
        if built.kind in ("chain", "star") and max_dist == 1:
            assert sorted(map(tuple, E.construction_links(built, 1).tolist())) == sorted(map(tuple, pairs.tolist()))


def test_small_builders_have_the_shapes_the_issue_names():
    n = E.SMALL_N
    b = E.bridged(n)
    assert sorted(set(b.labels[0].tolist())) == [0, 1, n - 1] and not b.labels[1].any()
    assert np.array_equal(E.chain(n, n + 4, "identity").labels[0], np.arange(n))
    assert E.star(n, n + 4, n - 1).logical[n - 1] == 0 and E.star(n, n + 4, 0).logical[0] == 0
    far = E.chain(n + 1, n + 4, "mod77")
    at = np.argsort(far.logical)
    assert (np.abs(at[1:] // 64 - at[:-1] // 64) >= 1).all()           # neighbours of the chain lie in different tiles


@pytest.mark.parametrize("name, built", contended_cases(), ids=[c[0] for c in contended_cases()])
def test_sampled_rows_of_a_contended_builder(name, built):
    """64 rows against all others at the GPU's size (every pair takes about a minute and is not wanted)"""
    rows = built.rows
    n = len(rows)
    assert rows.shape == (E.CONTENDED_N, E.CONTENDED_NCHAR)
    at = np.argsort(built.logical)
    sample = set(np.random.default_rng(5).choice(n, size=58, replace=False).tolist()) | {0, n - 1, 63, 64, int(at[0]), int(at[n - 1])}
    for p in sorted(sample)[:64]:
        assert np.array_equal(byte_distances(rows, p), E.distances_from(built, p)), (name, p)
    assert not built.labels[1].any() and built.links[1] == n - 1
    assert np.array_equal(built.labels[0], np.arange(n)) and built.links[0] == 0
    pairs = E.construction_links(built, 1)
    assert len(pairs) == n - 1 and (pairs[:, 0] < pairs[:, 1]).all()
    assert not K.components(n, pairs).any()


def test_contended_dense_and_bridged():
    n = E.CONTENDED_N
    for built in (E.dense(n), E.bridged(n)):
        rows = built.rows
        assert rows.shape == (n, 33)
        for p in (0, 1, 2, 63, 64, n - 2, n - 1):
            assert np.array_equal(byte_distances(rows, p), E.distances_from(built, p))
    b = E.bridged(n)
    assert sorted(set(b.labels[0].tolist())) == [0, 1, n - 1] and not b.labels[1].any()
    assert b.links[0] == 2080 * 2079 // 2 + 2079 * 2078 // 2 and b.links[1] == b.links[0] + n - 1
    assert (n + 63) // 64 == 65 and 32 * ((65 + 3) // 4) == 544        # column tiles; blocks of the first launch's 1 024 rows under the snp metric


def test_cuts_cover_every_pair_once():
    n = E.CONTENDED_N
    for calls in (E.bands_reversed(n), E.quadrants(n)):
        seen = np.zeros((n, n), dtype=np.uint8)
        for rows, cols in calls:
            c0, nc = cols or (0, n)
            seen[rows[0]:rows[0] + rows[1], c0:c0 + nc] += 1
        assert (seen == 1).all()


# ---- A: the argument (a model of the forest, NOT the compiled kernel)
def model_runs(n_runs, seed):
    rng = np.random.default_rng(seed)
    for k in range(n_runs):
        kind = E.MODEL_KINDS[k % len(E.MODEL_KINDS)]
        n = int(rng.integers(3, 41))
        yield kind, n, E.model_graph(kind, n, rng), int(rng.integers(0, 2 ** 31))


def test_the_forest_model_gives_the_components_under_every_interleaving_tried():
    """This tests the ARGUMENT of kernels_pairs.inc and DESIGN.md 4.12, not the compiled kernel: pairs_link_root and pairs_link_hits
    restated in Python one memory operation at a time (pair_edges.forest_model), the next lane picked at random, every load free to
    return any value its cell ever held, CAS and atomicMin on the current value.  300 interleavings over chains, stars, cliques and
    sparse random graphs of up to 40 nodes, a column's rows split over several lanes: the labels always equal pair_link.components."""
    for kind, n, edges, seed in model_runs(300, 97):
        want = K.components(n, edges)
        got = E.forest_model(n, edges, seed)
        assert np.array_equal(got, want), (kind, n, edges, seed)


def lost_hook_case():
    """two lanes that hook the same root at the same time: 0 - 2 and 1 - 2 (one component), column 2's two rows on a lane each"""
    return 3, [(0, 2), (1, 2)], [(2, [0]), (2, [1])]


def test_the_model_sees_a_lost_hook():
    """The same model with the CAS replaced by load, compare, store loses a hook under a fixed interleaving and, over the runs of the test
    above, under some of them; with the CAS every one of them is right.  That is the evidence that the model can see the fault the
    argument is about."""
    n, edges, lanes = lost_hook_case()
    want = K.components(n, edges)
    assert not want.any()
    assert not np.array_equal(E.forest_model(n, edges, E.LOST_HOOK_SEED, atomic_cas=False, lanes=lanes), want)
    assert all(np.array_equal(E.forest_model(n, edges, s, lanes=lanes), want) for s in range(200))
    lost = 0
    for kind, m, e, seed in model_runs(300, 97):
        lost += not np.array_equal(E.forest_model(m, e, seed, atomic_cas=False), K.components(m, e))
    assert lost > 0


# ---- B: the dirtied tiles
@pytest.mark.parametrize("name", ["awkward130x129", "synth130"])
def test_dirtied_tiles_keep_every_bit_that_counts(name):
    seqs, nchar = D.case(name)
    n = len(seqs)
    planes, _non_n = P.pack_tiles(seqs, nchar)
    W4 = ((nchar + 31) // 32 + 3) // 4
    keep = D.window_masks(W4 * 4, nchar, 0).reshape(W4, 1, 1, 4)
    view = lambda x: x.reshape(-1).view(np.uint32).reshape(-1, W4, 4, 64, 4)
    clean = view(planes)
    assert not (clean & ~keep).any() and not clean[-1, :, :, n % 64:, :].any()          # what this library packs is clean
    for how in ("lanes", "bits", "both"):
        d = view(E.dirty(planes, n, nchar, how))
        real = np.ones((clean.shape[0], 64), dtype=bool)
        real[-1, n % 64:] = False
        real = real[:, None, None, :, None]
        assert np.array_equal((d & keep)[np.broadcast_to(real, d.shape)], clean[np.broadcast_to(real, d.shape)]), how
        if how != "lanes":
            assert (d & ~keep).any(axis=(1, 2, 4)).all(), how                             # every lane has stale bits past nchar
        else:
            assert np.array_equal(d[:-1], clean[:-1]) and not (d & ~keep)[-1, :, :, :n % 64, :].any()
        if how != "bits":
            assert d[-1, :, :, n % 64:, :].any(axis=(0, 1, 3)).all(), how                 # every lane past the last row holds something
        assert np.array_equal(E.dirty(planes, n, nchar, how), d.view(np.uint8).reshape(planes.shape))      # a fixed seed


# ---- C: the database of the launch tests
def test_launch_database_and_the_uvaia_restatement():
    rows = E.launch_rows()
    n = E.LAUNCH_N
    assert rows.shape == (n, E.LAUNCH_NCHAR)
    # the matrix-product restatement equals the plane counters wherever those are computed: the band over the first launch edge and the last rows
    floor = E.launch_floor()
    assert floor <= 31

    def in_band(pairs, first, count):
        return sorted(map(tuple, pairs[(pairs[:, 0] >= first) & (pairs[:, 0] < first + count)].tolist()))
    for first, count in ((0, 1030), (8185, 15)):
        c = E.launch_counts(first, count)
        for max_dist, fl in ((1, 0), (3, 0), (1, floor), (0, 31)):
            want = E.band_links(c, first, "uvaia", max_dist, fl)
            assert in_band(E.launch_links("uvaia", max_dist, fl), first, count) == sorted(map(tuple, want.tolist())), (first, max_dist, fl)
        want = E.band_links(c, first, "snp", 1)
        assert in_band(E.launch_links("snp", 1), first, count) == sorted(map(tuple, want.tolist()))
    # the family is one cluster, its links cross both launch edges, and the floor bites: the copies of row 0 link no more
    fam = E.LAUNCH_FAMILY
    for fl in (0, floor):
        pairs = E.launch_links("uvaia", 1, fl)
        labels = K.components(n, pairs)
        assert all(labels[p] == fam[0] for p in fam) and int((labels == fam[0]).sum()) == len(fam)
        assert set(zip(fam, fam[1:])) <= set(map(tuple, pairs.tolist()))
        assert int((labels == 0).sum()) >= 207 if fl == 0 else labels[1] == 1
    assert 0 < len(E.launch_links("uvaia", 1, floor)) < len(E.launch_links("uvaia", 1, 0)) - 20000


@pytest.mark.parametrize("name", ["awkward9x129", "special129", "synth130"])
def test_the_uvaia_restatement_on_every_code(name):
    seqs, nchar = D.case(name)
    rows = np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), -1)
    for trim in (0, 33):
        c = D.plane_counts_of(seqs, nchar, trim)
        some = sorted(set(np.percentile(D.uvaia(c), (0, 25, 50)).astype(int).tolist()))
        for max_dist in some:
            for floor in (0, int(np.median(c[..., 3]))):
                want = E.band_links(c, 0, "uvaia", max_dist, floor)
                got = E.uvaia_links_of_bytes(rows, trim, max_dist, floor, block=64)
                assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist())), (trim, max_dist, floor)


def test_plane_counts_of_takes_a_row_range():
    seqs, nchar = D.case("synth130")
    whole = D.plane_counts_of(seqs, nchar, trim=1)
    assert np.array_equal(D.plane_counts_of(seqs, nchar, trim=1, rows=(60, 10)), whole[60:70])
    assert np.array_equal(D.plane_counts_of(seqs, nchar, trim=1, rows=7), whole[:7])
    assert D.plane_counts_of(seqs, nchar, rows=(130, 0)).shape == (0, 130, 5)


# ---- D: the query set of the one- and two-site engines
def test_the_short_query_is_what_the_preparation_gives_where_it_gives_anything():
    for nchar in (5, 33):
        q, s = O.Query([F.random_acgt(nchar, 3)], ["q0"]), E.short_query(nchar)
        assert q.ntax == 1 and (q.seqs, q.consensus, q.trim, q.acgt) == (s.seqs, s.consensus, s.trim, s.acgt)
        assert all(np.array_equal(a, b) for a, b in zip((q.idx_c, q.idx_m, q.idx), (s.idx_c, s.idx_m, s.idx)))
    assert D.dummy_query(4).ntax == 0 and D.dummy_query(5).ntax == 2
    assert [len(E.short_query(n).consensus) for n in (1, 2)] == [1, 2]
