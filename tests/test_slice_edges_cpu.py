"""The inputs of tests/slice_edges.py do what they are built for, shown with the oracle alone (no GPU): the restated planner gives every case the
slices of the issue's table and reaches each of the planner's five rules, the query sets have a constant-and-complete column or none as the case
says, every window of 8 192 stream positions holds an admission, the pair at every slice boundary stays in the final heaps with two ordinals and one
score, and in case e the pool boundary decides results."""
import numpy as np
import pytest

import slice_edges as S

KEYS = list(S.CASES)
MODES = [False, True]


def test_the_restated_planner_gives_the_table_and_every_rule_is_reached():
    for key, c in S.CASES.items():
        for acgt in MODES:
            pl = S.case_plan(key, acgt, 1 if c.cons else 0)
            assert tuple(s[1] for s in pl) == c.lengths, (key, acgt)
            assert pl[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(pl, pl[1:])) and pl[-1][0] + pl[-1][1] == c.n, key
    L = {k: c.lengths for k, c in S.CASES.items()}
    nqt = {k: (c.nq + 15) // 16 for k, c in S.CASES.items()}
    # 1. query-tile scaling: one tile in a -- without it 163 877 references were 13 slices of half the 63-tile length --, 63 tiles in g: none
    assert nqt["a"] == 1 and len(L["a"]) == 3 and (S.CASES["a"].n + S.SUBSLICE // 4) // (S.SUBSLICE // 2) == 13
    assert nqt["g"] == S.FULL_NQT and len(L["g"]) == (S.CASES["g"].n + S.SUBSLICE // 2) // S.SUBSLICE == 3
    scaled = (S.SUBSLICE // 2 * 63 // nqt["d"] + 63) // 64 * 64
    assert nqt["d"] == S.QUARTER_NQT and len(L["d"]) == 4 and abs(L["d"][1] - scaled) < scaled // 100            # two middles of about one scaled length
    # 2. the quarter rule: a quarter of a's pool is below 65 536, so its slices come from that floor (three of them, not four)
    assert (S.CASES["a"].n + 3) // 4 < S.QUARTER_MIN and sum(L["a"]) == S.CASES["a"].n
    assert L["c"][1] == 174784 and (S.CASES["c"].n + 3) // 4 > S.QUARTER_MIN      # c's middles: a quarter of the pool decides how many
    # 3. head / middle / pre / tail
    for k in "bcdf":
        assert L[k][0] == S.HEAD and L[k][-1] == S.TAIL and S.CASES[k].n >= S.HEAD_TAIL_POOL and nqt[k] < S.HEAD_TAIL_NQT, k
        assert all(x not in (S.HEAD, S.PRE) for x in (L[k][1:-2] if k == "c" else L[k][1:-1])), k
    assert L["c"][-2] == S.PRE and S.CASES["c"].n >= S.PRE_POOL and nqt["c"] < S.PRE_NQT
    assert S.PRE not in L["b"] and S.CASES["b"].n < S.PRE_POOL
    assert S.PRE not in L["d"] and S.CASES["d"].n < S.PRE_POOL and nqt["d"] >= S.PRE_NQT
    assert S.CASES["a"].n < S.HEAD_TAIL_POOL and S.CASES["e"].pool < S.HEAD_TAIL_POOL
    # slices that follow a boundary inside a tile: the launch before them scanned that tile too
    for k in "bcdef":
        assert any(b % 64 for b in S.boundaries(k)), k
    # 4. the 70 % first slice
    for k, lens in (("a", L["a"]), ("g", L["g"]), ("e", L["e"][:4]), ("e", L["e"][4:8])):
        assert lens[0] < min(lens[1:-1]) and lens[0] % 64 == 0 and abs(lens[0] - 0.7 * sum(lens) / len(lens)) < 128, k
    # 5. plain near-equal slices: e's pool of 37; and the pool that is cut (e) against the pool that is ignored (f) over the same references
    assert L["e"][8] == 37 and S.CASES["e"].n == S.CASES["f"].n and S.CASES["e"].pool == S.CASES["f"].pool and len(L["f"]) == 5
    pools = [s for s in S.case_plan("e", False, 1) if s[2]]
    assert [s[0] for s in pools] == [0, 300000, 600000]
    assert [s[2] for s in S.case_plan("f", False, 0)] == [True, False, False, False, False]


def test_the_restated_planner_tiles_every_range_it_is_asked_for():
    """(the invariants the device file asks of uvaia_gpu_search_plan, asked of the restatement over a small grid)"""
    for nq in (1, 48, 49, 257, 513, 992, 993):
        for cons in (0, 1):
            for sub in (0, 64, 448):
                for first in (0, 100):
                    for n in (1, 65, 62757, 8 * 65536 - 1, 12 * 65536 + 1):
                        for pool in (63, 100, 65536, n):
                            pl = S.plan(first, n, pool, nq, cons, False, subslice_refs=sub)
                            assert pl[0][0] == first and pl[-1][0] + pl[-1][1] == first + n
                            assert all(a[0] + a[1] == b[0] for a, b in zip(pl, pl[1:])) and all(s[1] >= 1 for s in pl)
                            if cons:
                                assert all(s[2] == ((s[0] - first) % pool == 0) and (s[0] - first) // pool == (s[0] + s[1] - 1 - first) // pool for s in pl)
                            else:
                                assert [s[2] for s in pl] == [True] + [False] * (len(pl) - 1)


@pytest.mark.parametrize("key", KEYS)
def test_query_sets_have_a_constant_and_complete_column_or_none(key):
    for acgt in MODES:
        q = S.query(key, acgt)
        assert q.ntax == S.CASES[key].nq
        assert (len(q.idx_c) > 0) == S.CASES[key].cons, (key, acgt, len(q.idx_c))
        assert len(q.idx) > 0
    assert S.refs(key).shape == (S.CASES[key].n, S.NCHAR) and S.NCHAR <= 512


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("acgt", MODES)
def test_every_window_holds_an_admission_and_every_boundary_a_pair(key, acgt):
    c, g = S.CASES[key], S.gold(key, acgt)
    assert g.n_seen == c.n and g.n_lowqual == 0
    assert S.longest_gap(g.saved, c.n) < S.WINDOW, (key, acgt)
    pl = S.case_plan(key, acgt, 1 if c.cons else 0)
    saved = np.asarray(g.saved)
    for f, n, _ in pl:                                   # so every slice longer than a window holds one
        if n > S.WINDOW:
            assert ((saved >= f) & (saved < f + n)).any(), (key, f, n)
    rows = S.want_rows(g)
    arr = S.refs(key)
    assert 1 <= len(S.boundaries(key)) <= (S.NBEST - 8) // 2
    for b in S.boundaries(key):
        assert np.array_equal(arr[b - 1], arr[b]) and not np.array_equal(arr[b], arr[b + 1] if b + 1 < c.n else arr[b - 2])
        assert b - 1 in saved and b in saved
        for iq, r in enumerate(rows):                    # every query keeps both to the end: same six scores, ordinals b - 1 and b
            by_ord = {o: s for s, o in r}
            assert b - 1 in by_ord and b in by_ord and by_ord[b - 1] == by_ord[b], (key, acgt, b, iq)
    # the worst kept entry is never one of a pair: the heaps still turn over at the end
    assert all(len(r) == S.NBEST for r in rows)


@pytest.mark.parametrize("acgt", MODES)
def test_case_e_the_pool_boundary_decides_results(acgt):
    c = S.CASES["e"]
    g = S.gold("e", acgt)
    one_pool = S.run_oracle("e", acgt, pool=c.n)
    assert S.want_rows(one_pool) != S.want_rows(g) and not np.array_equal(one_pool.saved, g.saved)
    # ... through references of the second pool: the first pool alone gives the same either way
    first_pool = np.asarray(g.saved) < c.pool
    assert np.array_equal(np.asarray(g.saved)[first_pool], np.asarray(one_pool.saved)[np.asarray(one_pool.saved) < c.pool])
    second = lambda s: set(int(x) for x in s if c.pool <= x < 2 * c.pool)
    assert second(g.saved) != second(one_pool.saved)
    # a tolerance rises inside the first pool, behind its first slice: the snapshot of the second pool is not the one a replay of that
    # slice would leave (the tolerances at the ends of the first pool's slices, from runs of the oracle over those prefixes)
    ends = np.cumsum(c.lengths[:4])
    assert ends[-1] == c.pool
    T = np.array([S.run_oracle("e", acgt, n=int(e)).final_T for e in ends])
    assert (np.diff(T, axis=0) > 0).any(), T
    assert T[-1].max() != T[0].max(), T


def test_the_same_references_without_a_constant_column_ignore_the_pool():
    """case f: the oracle's answer does not depend on the pool, which is what lets the planner lay one plan over the whole range"""
    c = S.CASES["f"]
    g = S.gold("f", False)
    one_pool = S.run_oracle("f", False, pool=c.n)
    assert S.want_rows(one_pool) == S.want_rows(g) and np.array_equal(one_pool.saved, g.saved) and one_pool.final_T == g.final_T
