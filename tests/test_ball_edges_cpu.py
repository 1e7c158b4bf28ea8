"""The inputs of tests/ball_edges.py, on the CPU: the oracle prepares every query set to the index sizes and the query order the builders
intend, every reference takes the stage it is built for (shown through ball_edges.stage, gather_layout and running), and the model's own
answer equals the oracle's cq->mindist for every reference, so what the model says about an input can be relied on.  The device runs the
same inputs in tests/test_ball_edges_gpu.py."""
import collections

import numpy as np
import pytest

import ball_edges as BE

MODES = [False, True]
MODE_IDS = ["default", "acgt"]


def check_model(q, refs, radius):
    """the model against the oracle on these references; returns the stages"""
    want, _ = q.ball(refs, ambig_r=0.001)
    st = [BE.stage(q, r, radius) for r in refs]
    assert [BE.answer(s, radius) for s in st] == list(want)
    return st, want


def check_qset(key, q):
    qs = BE.qset(key)
    assert q.ntax == len(qs.seqs), key                              # no query is pruned
    assert sorted(q.names) == sorted(qs.names)
    assert len(q.idx) == qs.n_idx and len(q.idx_m) == qs.n_idx_m, (key, len(q.idx), len(q.idx_m))
    assert len(q.idx_c) + len(q.idx_m) + len(q.idx) == qs.nchar          # no column is N in every query


# ---------------------------------------------------------------------------------------------------------------------------- A
def test_a_cases_cover_the_listed_column_counts_and_placements():
    assert sorted(set(c.n_idx for c in BE.A_CASES if c.nchar == 2000)) == [0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 640]
    places = collections.Counter(c.placement for c in BE.A_CASES)
    assert all(places[p] >= 3 for p in ("spread", "packed", "ends", "last-group", "spread-hot", "hot-above", "hot-interleaved"))
    assert set(c.nchar for c in BE.A_CASES) == {2000, 129, 100}
    for case in BE.A_CASES:
        cols, hot = BE.a_columns(case)
        if case.placement in ("packed", "hot-above", "hot-interleaved"):
            w = collections.Counter(int(c) // BE.WORD_COLS for c in cols)              # whole words, but for the last one
            assert sorted(w.values(), reverse=True)[:len(w) - 1] == [BE.WORD_COLS] * (len(w) - 1) and len(w) == -(-case.n_idx // BE.WORD_COLS)
        if case.placement == "ends":
            assert cols[0] == 0 and cols[-1] == case.nchar - 1
        if case.placement == "last-group":
            assert set(int(c) // BE.GROUP_COLS for c in cols) == {(case.nchar - 1) // BE.GROUP_COLS}
        if case.placement == "hot-above":
            assert hot.min() > np.setdiff1d(cols, hot).max()
        if case.placement == "hot-interleaved":                                         # hot and cold words alternate
            kind = [int(c) in set(hot.tolist()) for c in cols[::BE.WORD_COLS][:16]]
            assert kind == [True, False] * 8
    c129 = next(c for c in BE.A_CASES if c.nchar == 129)
    assert 128 in BE.a_columns(c129)[0]                                                  # the second word group's only site is gathered


@pytest.mark.parametrize("acgt", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", BE.A_NAMES)
def test_a_index_sizes_layout_and_references_that_go_on(name, acgt):
    case = BE.A_CASES[BE.A_NAMES.index(name)]
    q, refs = BE.group_a(name, acgt)
    check_qset("A-" + name, q)
    cols, hot = BE.a_columns(case)
    assert len(q.idx) == case.n_idx and list(q.idx) == list(cols) and len(q.idx_m) == case.n_idx_m
    lay = BE.gather_layout(q)
    assert (lay.NH4, lay.NG4) == BE.a_expected_layout(case)
    if case.n_idx >= 2 * BE.BALL_HOT_COLS:                                               # the hot columns are the designed ones
        assert lay.NH4 == 2 and sorted(lay.order[:BE.BALL_HOT_COLS]) == sorted(hot.tolist())
        assert lay.score[np.isin(cols, hot)].min() > lay.score[~np.isin(cols, hot)].max()
        assert list(lay.order) != list(cols)
    else:
        assert lay.NH4 == 0 and list(lay.order) == list(cols)
    assert len(refs) == BE.A_NREF
    st, want = check_model(q, refs, BE.A_RADIUS)
    asked = [i for i, s in enumerate(st) if s.asks]
    assert len(asked) >= 100
    assert len(set(int(want[i]) for i in asked)) >= 3
    if case.n_idx:                                                                       # the walk ends at a query for some and at none for others
        assert any(st[i].first_query is None for i in asked) and any(st[i].first_query is not None for i in asked)


def test_a_ambiguity_codes_count_by_text_in_default_mode_only():
    """the same references, the two modes: where a reference holds R, Y, K or M at a column of idx the default mode counts it and --acgt
    does not, so some answers differ"""
    differ = 0
    for name in ("n33-spread", "n257-packed", "n513-hot-above"):
        (q0, r0), (q1, r1) = BE.group_a(name, False), BE.group_a(name, True)
        assert r0 == r1 and list(q0.idx) == list(q1.idx) and q0.seqs == q1.seqs
        assert any(c in r for r in r0 for c in b"RYKM") and any(b"-" in r for r in r0)
        differ += int((q0.ball(r0, ambig_r=0.001)[0] != q1.ball(r1, ambig_r=0.001)[0]).sum())
    assert differ > 0


# ---------------------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("acgt", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nq", BE.B_NQ)
def test_b_first_query_below_the_limit(nq, acgt):
    q, cases = BE.group_b(nq, acgt)
    check_qset("B-%d" % nq, q)
    assert q.ntax == nq
    if nq >= 15:
        assert q.names != list(BE.qset("B-%d" % nq).names)                               # preparation reorders: positions are read back
    names = [c.name for c in cases]
    for p in BE.b_positions(nq):
        if nq > 1:
            assert "only-%d-at-0" % p in names and "only-%d-at-limit-1" % p in names
    if nq == 33:
        assert "first-3-not-nearest-20" in names
    if nq >= 15:
        assert "first-3-not-nearest-9" in names
    st, want = check_model(q, [c.ref for c in cases], BE.B_RADIUS)
    for c, s, w in zip(cases, st, want):
        assert s.asks and (s.first_query, s.d_first) == (c.first_query, c.d_first), (c.name, s)
        limit = BE.B_RADIUS - s.md
        d = BE.running(q, c.ref)[:, -1]
        if c.name.startswith("only-"):                                                   # every other query sits exactly at the limit
            assert sorted(set(d.tolist())) == sorted({c.d_first, limit}) or nq == 1
        if c.name == "none-below":
            assert d.min() == limit and w == BE.B_RADIUS
        if c.name.startswith("first-"):                                                  # the nearest query is a later one
            late = int(c.name.rsplit("-", 1)[1])
            assert d[late] == 0 and d[c.first_query] == limit - 1 and late > c.first_query and w == s.md + limit - 1
            if c.name == "first-3-not-nearest-9":
                assert c.first_query // BE.QTB == late // BE.QTB                         # both in one tile of 16 ...
            if c.name in ("first-3-not-nearest-20", "first-15-not-nearest-16"):
                assert c.first_query // BE.QTB != late // BE.QTB                         # ... or the keys of two waves meet in atomicMin


# ---------------------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("acgt", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(BE.C_CASES))
def test_c_one_lane_keeps_one_query_alive(name, acgt):
    q, refs = BE.group_c(name, acgt)
    check_qset("C-" + name, q)
    lay = BE.gather_layout(q)
    assert (lay.n_hot, lay.NG4) == ((0, 4) if name == "cold511" else (256, 5))
    st, _ = check_model(q, refs, BE.C_RADIUS)
    assert len(refs) == BE.TILE + 1 and all(s.asks and s.md == BE.C_RADIUS - BE.C_LIMIT for s in st)
    run = np.stack([BE.running(q, r) for r in refs])                                     # [lane, query, word group]
    below = run < BE.C_LIMIT
    for n in (BE.TILE, BE.TILE + 1):
        after0 = set(zip(*np.nonzero(below[:n, :, 0])))
        assert after0 == {(BE.C_LANE, BE.C_QUERY), (BE.C_LANE2, BE.C_QUERY2)}            # every other query leaves the scan after group 0
    assert below[BE.C_LANE, BE.C_QUERY].all()                                            # below its limit through the last word group ...
    assert run[BE.C_LANE, BE.C_QUERY, -1] == BE.C_LIMIT - 1 > run[BE.C_LANE, BE.C_QUERY, -2]   # ... in which it still counts
    assert list(below[BE.C_LANE2, BE.C_QUERY2]) == [True] + [False] * (lay.NG4 - 1)      # alive for one more group only
    assert (st[BE.C_LANE].first_query, st[BE.C_LANE].d_first) == (BE.C_QUERY, BE.C_LIMIT - 1)
    assert [s.first_query for i, s in enumerate(st) if i != BE.C_LANE] == [None] * BE.TILE


# ---------------------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("acgt", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("radius", BE.D_RADII)
def test_d_every_branch_of_ball_one(radius, acgt):
    q, refs = BE.group_d("main", acgt, radius)
    check_qset("D-main", q)
    assert (len(q.idx_c), len(q.idx_m), len(q.idx)) == BE.D_EXPECT["main"]
    st, _ = check_model(q, refs, radius)
    taken = collections.Counter(BE.branch(s, radius) for s in st)
    for b in ("first", "second", "doubled", "loop"):
        if b == "loop" and radius == 1:                                                  # md < 1 is md = 0, and 2 * 0 < 1: no reference can ask
            assert taken[b] == 0
        else:
            assert taken[b] >= 5, (radius, taken)
    R, seen = radius, set((s.dc, s.dm) for s in st)
    assert {(R - 1, 0), (R, 0), (R + 1, 0), (len(q.idx_c), 0), (0, R + 1), (0, 0)} <= seen
    assert {R - 1, R, R + 1} <= set(s.dc + s.dm for s in st if s.dc < R)
    assert {t for t in (R - 1, R, R + 1) if t % 2 == 0 and t // 2 < R} <= set(2 * s.md for s in st if s.md < R)     # (radius 1: md = 1 never gets there)
    assert any(any(c in r for c in b"RYKM") for r in refs)


@pytest.mark.parametrize("acgt", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", BE.D_SETS[1:])
def test_d_query_sets_without_one_or_both_constant_sets(name, acgt):
    for radius in BE.D_RADII:
        q, refs = BE.group_d(name, acgt, radius)
        check_qset("D-" + name, q)
        assert (len(q.idx_c), len(q.idx_m), len(q.idx)) == BE.D_EXPECT[name]
        st, _ = check_model(q, refs, radius)
        taken = collections.Counter(BE.branch(s, radius) for s in st)
        if name == "all-polymorphic":                                                    # nothing to be distant from: md = 0 for everyone
            assert set(taken) == {"doubled"}
        else:
            assert taken["doubled"] >= 5 and (radius == 1 or taken["loop"] >= 5)
            assert taken["first" if name == "no-idx-m" else "second"] >= 5


# ---------------------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("acgt", MODES, ids=MODE_IDS)
def test_e_subsets_send_exactly_the_wanted_number_on(acgt):
    q, refs, asks = BE.group_e(acgt)
    check_qset("E", q)
    assert len(refs) == BE.E_NREF > BE.MAX_POOL
    st, _ = check_model(q, refs, BE.E_RADIUS)
    assert [s.asks for s in st] == list(asks) and asks.sum() >= max(BE.E_COUNTS)
    assert sorted(BE.E_ORDER) == sorted(BE.E_COUNTS)
    assert [a > b for a, b in zip(BE.E_ORDER, BE.E_ORDER[1:])].count(True) >= 3           # short lists follow long ones
    for count in BE.E_COUNTS:
        for layout in ("scattered", "one-tile"):
            sub = BE.e_subset(asks, count, layout)
            assert len(sub) == len(set(sub)) == BE.E_SUBSET <= BE.MAX_POOL
            at = np.nonzero(asks[sub])[0]
            assert len(at) == count == BE.n_asked(q, [refs[i] for i in sub], BE.E_RADIUS)
            tiles = set(int(k) // BE.TILE for k in at)
            if layout == "one-tile":
                assert len(tiles) == -(-count // BE.TILE)
            elif count >= BE.TILE:
                assert len(tiles) == -(-BE.E_SUBSET // BE.TILE)
    # more than one block of four tiles in stage 1 (the subset) and in the scan (the longest lists), and lists that end inside a block
    assert -(-BE.E_SUBSET // BE.TILE) > BE.TILES_PER_BLOCK and -(-max(BE.E_COUNTS) // BE.TILE) == BE.TILES_PER_BLOCK + 1
    assert 0 < asks[:BE.E_FIRST_APPEND].sum() < BE.TILE < asks.sum()


# ---------------------------------------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("acgt", MODES, ids=MODE_IDS)
def test_f_ranges_start_and_end_inside_tiles(acgt):
    q, refs = BE.group_f(acgt)
    assert len(refs) == BE.MAX_POOL and refs[:BE.D_NREF] == BE.group_d("main", acgt, BE.F_RADIUS)[1]
    st, _ = check_model(q, refs, BE.F_RADIUS)
    assert BE.F_DB % BE.TILE == 8 and BE.F_DB // BE.TILE == 3
    assert any(a % BE.TILE and (a + n) % BE.TILE for a, n in BE.F_RANGES) and (100, 0) in BE.F_RANGES
    for a, n in BE.F_RANGES:
        assert a + n <= BE.F_DB
        k = sum(s.asks for s in st[a:a + n])
        assert k > 0 or n < BE.TILE - 1, (a, n, k)                                       # every range of some length sends some on
    taken = collections.Counter(BE.branch(s, BE.F_RADIUS) for s in st[:BE.F_DB])
    assert min(taken[b] for b in ("first", "second", "doubled", "loop")) >= 5
