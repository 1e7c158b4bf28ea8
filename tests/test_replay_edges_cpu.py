"""The inputs of tests/replay_edges.py, on the CPU: the oracle prepares every query set as the builders intend, and every input reaches the edge
it is built for -- shown from the oracle's pair scores (Query.allpairs), the oracle's answers to the stream and to prefixes of it, and the
model of replay_edges (MinHeap, walk2, walk3), whose own answer is held against the oracle's first, so that what it says about an input
can be relied on.  The device runs the same inputs in tests/test_replay_edges_gpu.py."""
import functools
import glob
import math
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import replay_edges as RE


def probe_scores(key, regime="replay3"):
    """the probe's untruncated score vectors against the case's references, as tuples"""
    q = RE.query(key, regime)
    s = q.allpairs(list(RE.CASES[key].refs))[:, RE.probe_index(key, regime), :]
    return [tuple(int(x) for x in r) for r in s]


def check_model(key, scores):
    """the model's search of the probe against the oracle's; returns (heap, trace)"""
    case = RE.CASES[key]
    g = RE.gold(key, "replay3")
    pi = RE.probe_index(key, "replay3")
    h, trace = RE.replay_model(scores, case.nbest, len(case.queries[0]))
    assert h.final() == RE.want_rows(g, pi + 1)[pi], key
    assert h.tolerance(len(case.queries[0])) == g.final_T[pi], key
    return h, trace


# ------------------------------------------------------------------------------------------------------------------------ all groups
def test_every_case_id_names_group_regime_and_edge():
    ids = [RE.run_id(k, r) for k, r in RE.runs()]
    assert len(set(ids)) == len(ids)
    assert all(i.split("-")[0] in "RGHKTSFC" and len(i.split("-")) >= 3 for i in ids)
    assert set(c.group for c in RE.CASES.values()) == set("RGHKTSFC")
    kernels = {g: set(RE.REGIMES[r].kernel for k, r in RE.runs(g)) for g in "RGHKTSFC"}
    assert {"replay", "replay2", "replay3"} <= kernels["C"]                 # (the lean kernel runs without a constant-and-complete column: nothing to cut)
    for g in "RHKF":                                                    # these groups run on all four kernels
        assert {"replay", "replay2", "lean", "replay3"} <= kernels[g], g
    assert {"replay2", "lean", "replay3"} <= kernels["G"] and {"replay2", "replay3"} <= kernels["T"] and {"replay2", "replay3"} <= kernels["S"]


def test_every_quoted_line_is_in_the_engine_sources():
    """the edge table and the copied constants quote the lines they mirror: a line that changes takes its quote, and the copy, with it"""
    def norm(t):
        return re.sub(r"\s+", " ", t).strip()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = norm(" ".join(open(f).read() for f in sorted(glob.glob(os.path.join(root, "uvaia_amd", "csrc", "*.inc")) + glob.glob(os.path.join(root, "uvaia_amd", "csrc", "*.hip")))))
    text = open(RE.__file__).read()
    head = text[:text.index("_ROT = np.arange")]                        # the module's docstring and its block of constants
    quotes = [x for x in re.findall(r"`([^`]+)`", head) if re.search(r"[();=\[<]", x)]
    assert len(quotes) >= 60
    missing = [x for x in quotes if norm(x) not in src]
    assert not missing, missing
    for name, line in (("D", "constexpr int D = 8;"), ("PD", "constexpr int PD = 4;"), ("BR", "constexpr int BR = 16;"), ("AMB_CAP", "constexpr int AMB_CAP = 11;")):
        assert line in quotes and int(line.split("=")[1].strip(" ;")) == getattr(RE, name)
    assert "{%s}" % ", ".join(str(x) for x in RE.TB8_THR) in " ".join(quotes) and "k <= %d" % RE.MC_LIMIT in " ".join(quotes)
    assert "c->nchar > %d" % RE.WIDE_ABOVE in " ".join(quotes) and "r < %d; r++) fetch_bounds(r)" % RE.INITIAL_ROUNDS in " ".join(quotes)


@pytest.mark.parametrize("key", [k for k in RE.CASES if "nchar" not in RE.CASES[k].meta])
def test_query_sets_are_prepared_as_intended(key):
    case = RE.CASES[key]
    for name in case.regimes:
        nq = RE.REGIMES[name].nq
        seqs = RE.queries_for(case, name)
        q = RE.query(key, name)
        assert q.ntax == len(seqs) == (nq or len(case.queries)) and sorted(q.seqs) == sorted(seqs), (key, name)      # no query pruned
        if RE.REGIMES[name].kernel == "lean" or name == "replay2-q256":
            assert len(q.idx_c) == 0, (key, name)                       # lean_replay_context: no constant-and-complete column
            assert (case.nbest <= RE.MC_LIMIT) == (name == "lean")
        if RE.REGIMES[name].kernel == "replay3":
            assert q.ntax <= 32


# ---------------------------------------------------------------------------------------------------------------------------- R
def test_r_stream_lengths_sit_at_the_round_edges():
    rounds = {nt: -(-nt // RE.TILE) for nt in RE.R_TILES_3}
    assert rounds == {1: 1, 64: 1, 65: 2, 256: RE.PD, 257: RE.PD + 1, 321: RE.PD + 2, 576: RE.INITIAL_ROUNDS, 577: RE.INITIAL_ROUNDS + 1,
                      833: 14, 1024: RE.BR, 1025: RE.BR + 1, 1089: RE.BR + 2, 2112: 2 * RE.BR + 1}
    # 257 / 577 / 833 / 1025: the last round holds one tile, so 63 lanes of its bounds lie past the slice
    assert all(nt % RE.TILE == 1 for nt in (65, 257, 321, 577, 833, 1025, 1089))
    n, at = RE.r_plants(2112)
    assert n == 2111 * RE.TILE + RE.R_LAST and set(o // (RE.TILE * RE.TILE) for o in at) == set(RE.R_ROUNDS)
    assert set(r & (RE.BR - 1) for r in RE.R_ROUNDS if r >= RE.BR) == {0, 1, 15}            # the ring's slots used a second and a third time
    assert {3, 15, 31} <= set(RE.R_ROUNDS) and {4, 16, 32} <= set(RE.R_ROUNDS)              # the rounds that refill ((rnd & 3) == 3) and the ones after


@pytest.mark.parametrize("nt", RE.R_TILES_3)
def test_r_only_the_plants_enter(nt):
    key = "R-tiles%d" % nt
    case = RE.CASES[key]
    at = case.meta["plants"]
    assert len(case.refs) == case.meta["n_ref"] == (nt - 1) * RE.TILE + RE.R_LAST
    lanes = set(o % RE.TILE for o in at)
    assert 0 in lanes and (nt == 1 or RE.TILE - 1 in lanes) and at[-1] == len(case.refs) - 1
    g = RE.gold(key, "replay3")
    assert list(g.saved) == at                                        # every plant, and no other reference of any round
    assert all(len(r) == RE.R_NBEST for r in g.rows)
    s = probe_scores(key)
    for a, b in zip(at, at[1:]):
        assert RE.lex_better(s[b], s[a]) and RE.mismatches(s[b]) == 2   # each displaces the one before
    assert [o for o, _n, _s in g.rows[0]] == at[::-1][:RE.R_NBEST]
    tiles = set(o // RE.TILE for o in at)
    if nt >= RE.TILE:
        assert len(tiles) < 0.05 * nt                                 # what lets the device test bound replay3's opened tiles
    if nt in RE.R_TILES_2:
        assert list(RE.gold(key, "lean").saved) == at
    if nt <= 1089:                                                    # the model's walks open the plants' tiles and no other
        ent, regroups, _f, opened = RE.walk2(s, RE.R_NBEST, RE.R_NCHAR)
        assert ent == at and not regroups and set(opened) - set(range(RE.D)) == tiles - set(range(RE.D))
        for half in (32, 8):
            ent, late, opened = RE.walk3(s, RE.R_NBEST, RE.R_NCHAR, half)
            assert ent == at and not late and set(opened) - set(range(half)) == tiles - set(range(half))


# ---------------------------------------------------------------------------------------------------------------------------- G
@pytest.mark.parametrize("key", RE.keys("G"))
def test_g_the_skipped_tile_becomes_needed(key):
    case = RE.CASES[key]
    m = case.meta
    s = probe_scores(key)
    h, trace = check_model(key, s)
    nchar = RE.G_NCHAR
    ent2, regroups, fells, opened2 = RE.walk2(s, RE.G_NBEST, nchar)
    assert ent2 == [o for o, t in enumerate(trace) if t[0]]            # the walks lose nothing
    u = m["u"]
    T_before, T_after = trace[u * RE.TILE - 1][1], trace[(u + 1) * RE.TILE - 1][1]
    if m.get("fall"):
        assert (T_before, T_after) == (10, 2)
        assert fells[-1] == (u, m["x"])                               # in flight, no longer needed: their ballots come out empty
        five = [t * RE.TILE + (t - 60) for t in m["x"]]
        assert all(RE.mismatches(s[o]) == 5 and RE.lex_better(s[o], s[1]) and not trace[o][0] for o in five)   # they would have entered before
        for half in (32, 16, 8):
            ent3, late, opened3 = RE.walk3(s, RE.G_NBEST, nchar, half)
            assert ent3 == ent2 and not late and not set(m["x"]) & set(opened3)
        return
    x = m["x"]
    xo = next(o for o in range(x * RE.TILE, (x + 1) * RE.TILE) if trace[o][0])
    assert (T_before, T_after) == (3, 10) and RE.mismatches(s[xo]) == 5 and xo in RE.gold(key, "replay3").saved
    tb = RE.tile_bounds(s)
    assert tb[x][0] >= T_before and tb[x][2][RE.tb8_index(T_before)] == 0      # not needed before the jump under either kind of bound ...
    assert tb[x][0] < T_after and tb[x][1] >= trace[(u + 1) * RE.TILE - 1][2]   # ... needed after it
    if "regroup" in m:
        in_flight = min(m["decoys"], RE.D - 1)                          # decoys behind u in its group of D
        assert regroups == ([(u, x, in_flight)] if m["regroup"] else [])
        decoys = [t for t in opened2 if u < t and t != x]               # a regroup drops them (the new state does not need them); else the ones in flight are opened
        assert len(decoys) == (0 if m["regroup"] else in_flight) and opened2.index(x) == opened2.index(u) + 1 + len(decoys)
        assert all(RE.tile_bounds(s)[t][0] < T_before and not any(trace[o][0] for o in range(t * RE.TILE, (t + 1) * RE.TILE)) for t in range(68, 68 + 2 * m["decoys"], 2))
    for half in (32, 16, 8):
        ent3, late, opened3 = RE.walk3(s, RE.G_NBEST, nchar, half)
        assert ent3 == ent2
        if m.get("half") == half:
            assert late == [x]
            hu, hx = u // half, x // half
            assert {"same-half": hx == hu, "next-half": hx == hu + 1 and x % half == 0 and x // RE.TILE == u // RE.TILE,
                    "next-round": x // RE.TILE == u // RE.TILE + 1}[m["late"]]


def test_g_covers_every_placement():
    metas = [RE.CASES[k].meta for k in RE.keys("G")]
    assert sorted((m["regroup"], len([1 for t in range(68, 84, 2)])) for m in metas if "regroup" in m).count((True, 8)) == 3
    assert sorted((m["late"], m["half"]) for m in metas if "late" in m) == sorted((w, h) for w in ("same-half", "next-half", "next-round") for h in (32, 16, 8))
    assert sum(1 for m in metas if m.get("fall")) == 1


# ---------------------------------------------------------------------------------------------------------------------------- H
@pytest.mark.parametrize("nbest", RE.H_NBEST)
def test_h_every_depth_ties_and_the_tie_rule_shows(nbest):
    key = "H-nbest%d" % nbest
    case = RE.CASES[key]
    assert len(case.refs) >= 3 * nbest
    s = probe_scores(key)
    assert len(set(s)) <= RE.H_CLASSES and len(set(RE.mismatches(x) for x in s)) == 1   # a small set of score vectors, one tolerance
    h, trace = check_model(key, s)
    k = max(2, nbest)
    deepest = int(math.log2(k))
    assert set(h.depths) == set(range(deepest + 1)), (sorted(set(h.depths)), deepest)   # from "stays the root" to the deepest leaf
    assert (deepest == 6) == (nbest in (64, 127)) and (nbest <= RE.MC_LIMIT or deepest == 7)
    assert h.tied_evictions >= 1
    wrong, _ = RE.replay_model(s, nbest, RE.H_NCHAR, prefer_right=True)
    assert [x[0] for x in wrong.final()] == [x[0] for x in h.final()]   # the same score vectors ...
    if k >= 3:                                                          # (a heap of two has no pair of children)
        assert [x[1] for x in wrong.final()] != [x[1] for x in h.final()]   # ... and other ordinals: the right child on ties cannot pass


# ---------------------------------------------------------------------------------------------------------------------------- K
@pytest.mark.parametrize("nbest", [1, 3])
@pytest.mark.parametrize("ladder", ["default", "acgt"])
def test_k_each_rung_ties_below_its_key_and_differs_by_one(ladder, nbest):
    acgt = ladder == "acgt"
    key, regime = ("K-acgt-ladder-nbest%d" % nbest, "replay2-acgt") if acgt else ("K-nbest%d" % nbest, "replay3")
    case = RE.CASES[key]
    q = RE.query(key, regime)
    assert set(RE.K_POLY) <= set(q.idx.tolist()) and RE.K_M in q.idx_m.tolist() and RE.K_MIS[0] in q.idx_c.tolist()
    pi = RE.probe_index(key, regime)
    s = probe_scores(key, regime)
    g = RE.gold(key, regime)
    h, trace = RE.replay_model(s, nbest, RE.K_NCHAR, acgt=acgt)
    assert h.final() == RE.want_rows(g, q.ntax)[pi] and h.tolerance(RE.K_NCHAR, acgt) == g.final_T[pi]     # the model's search is the oracle's
    refs = list(case.refs)
    seen = set()
    for (name, j, d, _a, _b, enters), (ia, ib) in zip(RE.K_LADDERS[ladder], RE.k_positions(nbest, ladder)):
        sa, sb = s[ia[0]], s[ib]
        assert all(s[o] == sa for o in ia) and len(ia) == max(2, nbest)
        if j is None:
            assert sb == sa
        else:
            assert sb[:j] == sa[:j] and sb[j] - sa[j] == d, (name, sa, sb)
            seen.add((j, d))
        T = trace[ib - 1][1]
        assert T == RE.mismatches(sa, acgt) + 1 == (4 if acgt else 5)   # the worst kept entry is A when B arrives
        before = O.search(q, refs[:ib], RE.names(ib), pool=ib, nbest=nbest, ambig_r=1.0)
        assert [tuple(x) for _o, _n, x in before.rows[pi]][-1] == sa and sorted(o for o, _n, _x in before.rows[pi])[-(max(2, nbest) - 1):] == ia[1:]
        after = O.search(q, refs[:ib + 1], RE.names(ib + 1), pool=ib + 1, nbest=nbest, ambig_r=1.0)
        assert (ib in [o for o, _n, _x in after.rows[pi]]) == enters == trace[ib][0], name
        assert enters == (RE.lex_better(sb, sa) and RE.mismatches(sb, acgt) < T), name
        if "at-the-gate" in name:
            assert RE.lex_better(sb, sa) and RE.mismatches(sb, acgt) == T
    assert seen >= {(j, d) for j in range(5 if acgt else 6) for d in (+1, -1)}
    if acgt:                                                            # keys 4 and 5 add up to the mismatches: no rung of its own for key 5
        assert all(x[4] + x[5] == x[1] - x[0] for x in s)


# ---------------------------------------------------------------------------------------------------------------------------- T
@pytest.mark.parametrize("key", RE.keys("T"))
def test_t_tolerances_on_both_sides_of_every_threshold(key):
    case = RE.CASES[key]
    m = case.meta
    t = m["t"]
    q = RE.query(key, "replay3")
    assert (len(q.idx_c) > 0) == m["cons"] and (m["cons"] or len(q.idx_c) == 0)
    s = probe_scores(key)
    h, trace = check_model(key, s)
    mm = [RE.mismatches(x) for x in s]
    assert mm[m["A"]] == mm[m["B"]] == mm[m["E"]] == t and mm[m["G"]] == t + 1 and mm[m["X"]] == m["x_mis"]
    T = t + 1
    assert trace[m["B"]][1] == T and trace[m["E"]][1] == T and h.tolerance(RE.T_NCHAR) == T
    assert trace[m["E"]][0] and s[m["E"]][0] == s[m["B"]][0] + 1                         # T - 1 mismatches, ahead on key 0: enters
    w = h.e[1][0]
    assert not trace[m["G"]][0] and RE.lex_better(s[m["G"]], w)                          # T mismatches, ahead on key 0: the gate alone refuses
    assert not trace[m["X"]][0] and RE.lex_better(s[m["X"]], w)
    assert [o for o, x in enumerate(trace) if x[0]] == [m["A"], m["B"], m["E"]]
    j = RE.tb8_index(T)
    thr = RE.TB8_THR[j] if j < len(RE.TB8_THR) else None
    assert (thr is None) == (t > RE.TB8_THR[-1]) and (thr is None or (thr >= t and (j == 0 or RE.TB8_THR[j - 1] < t)))
    counted = thr is None or m["x_mis"] <= thr
    assert counted == (t not in RE.TB8_THR)                                              # X's count is the next threshold above T - 1
    for half in (32, 8):
        ent, late, opened = RE.walk3(s, 1, RE.T_NCHAR, half)
        assert sorted(ent) == [m["A"], m["B"], m["E"]] and not late
        assert (1 not in opened) and (2 in opened) and ((3 in opened) == counted), (t, opened)
    ent, _r, _f, opened = RE.walk2(s, 1, RE.T_NCHAR)
    assert 2 in opened and sorted(ent) == [m["A"], m["B"], m["E"]]


def test_t_values_are_each_threshold_and_the_count_after_it():
    assert set(RE.T_VALUES) == set(RE.TB8_THR) | {x + 1 for x in RE.TB8_THR if x + 1 not in RE.TB8_THR} | {RE.TB8_THR[-1] + 2}
    assert sorted(c.meta["t"] for c in RE.CASES.values() if c.group == "T" and c.meta["cons"]) == sorted(RE.T_VALUES)


# ---------------------------------------------------------------------------------------------------------------------------- S
def _listed_words(seq):
    a = np.frombuffer(seq, dtype=np.uint8)
    amb = ~np.isin(a, np.frombuffer(b"ACGTN-", dtype=np.uint8))
    return set((np.nonzero(amb)[0] // 32).tolist())


@pytest.mark.parametrize("key", [k for k in RE.keys("S") if "cut" not in RE.CASES[k].meta])
def test_s_lists_of_exactly_the_intended_lengths(key):
    case = RE.CASES[key]
    m = case.meta
    probe = RE.rows(case.queries)[0]
    refs = list(case.refs)
    ql = _listed_words(probe)
    assert len(ql) == m["n_q"]
    s = probe_scores(key)
    g = RE.gold(key, "replay3")
    lens, shared_seen = set(), False
    for o, (n_r, shared) in zip(m["at"], m["kinds"]):
        rl = _listed_words(refs[o])
        assert len(rl) == n_r and bool(rl & ql) == (min(n_r, m["n_q"]) > 0 if shared else n_r + m["n_q"] > RE.S_WORDS)
        shared_seen |= bool(rl & ql)
        lens.add(n_r)
        assert RE.mismatches(s[o]) == RE.S_BAD + 0 and o in g.saved            # compared exactly, enters
        if shared and rl & ql:
            assert s[o][1] == s[o][0] + len(rl & ql)                                           # R under the probe's R: a text match beyond the ACGT ones
        if n_r:
            assert s[o][2] > s[o][1]                                           # R against A: a partial match
    overflow = max(lens) > RE.AMB_CAP
    assert m["dense"] == (overflow or m["n_q"] > RE.AMB_CAP)
    assert lens == ({RE.AMB_CAP + 1} if overflow else {0, 1, RE.AMB_CAP - 1, RE.AMB_CAP})
    if not overflow and 0 < m["n_q"]:
        assert shared_seen
    if not overflow and m["n_q"] == RE.AMB_CAP:
        assert any(n_r == RE.AMB_CAP for n_r, _s in m["kinds"])                # 11 + 11: 22 lanes of wave_iupac_request
    if not overflow and m["n_q"] == 1:
        assert (1, True) in m["kinds"]                                         # the shared word is the only listed word, on both sides


def test_s_counts_are_the_cap_and_its_neighbours():
    assert RE.S_COUNTS == (0, 1, RE.AMB_CAP - 1, RE.AMB_CAP, RE.AMB_CAP + 1) and RE.S_WORDS > RE.AMB_CAP + 1


@pytest.mark.parametrize("variant", ["cut", "cut-listed"])
def test_s_pairs_cut_at_the_snapshot_next_to_uncut_ones(variant):
    key = "S-%s-pool64" % variant
    case = RE.CASES[key]
    lay = case.meta["cut"]
    at = {v: [o for o, n in lay.items() if n == v] for v in set(lay.values())}
    q = RE.query(key, "replay3")
    more = 3 if case.meta["listed"] else 0                  # A against the probe's two R, and R against A: valid pairs without an ACGT match
    assert q.ntax == 1 and len(q.idx_c) == 128                  # one query: every column is constant and complete, the two of R too
    s = probe_scores(key)
    g = RE.gold(key, "replay3")
    saved = set(g.saved.tolist())
    nine, plant = at["nine"][0], at["plant"][0]
    assert {at["low"][0], nine, plant} <= saved
    early, late = at["five-early"], at["five-late"][0]
    assert all(plant < o and o // RE.TILE == plant // RE.TILE for o in early + [late])     # the same tile, behind the plant
    assert all(RE.mismatches(s[o]) == 5 + more and s[o][0] >= s[nine][0] for o in early + [late])  # uncut: upper-bound key 0 reaches the worst kept one
    assert late in saved and not set(early) & saved                                         # the cut scores decide
    row = {o: tuple(x) for o, _n, x in g.rows[0]}
    assert row[plant] == s[plant]                                                           # an uncut pair keeps its scores
    assert (late in row) == case.meta["listed"]                                             # (cut-listed: the cut pair stays to the end)
    refs = list(case.refs)
    before_late = O.search(q, refs[:late + 1], RE.names(late + 1), pool=64, nbest=2, ambig_r=1.0)
    cut = {o: tuple(x) for o, _n, x in before_late.rows[0]}[late]
    snap = RE.mismatches(s[at["low"][0]]) + 1
    assert snap == (5 if case.meta["listed"] else 3) and cut != s[late] and cut[3] < s[late][3]                      # entered with the counters cut at the snapshot
    if case.meta["listed"]:
        assert _listed_words(RE.rows(case.queries)[0]) == {1, 2} and _listed_words(refs[late]) == {1}     # a word on both lists
        assert cut[1] - cut[0] == 1 and cut[2] - cut[1] == 2                                # R under R once; R against A and A against the probe's other R
    g2 = RE.gold("S-%s-pool2" % variant, "replay3")
    assert set(g2.saved.tolist()) != saved                                                  # pools of 2 retake the snapshot: another answer


# ---------------------------------------------------------------------------------------------------------------------------- F
def test_f_ordinals_wrap_inside_a_tile_and_entries_come_from_every_tile():
    assert RE.F_ORDINALS == (2 ** 31 - 3, 2 ** 32 - 3, 2 ** 40) and RE.F_N == 2 * RE.TILE + 2
    for o0 in RE.F_ORDINALS:
        key = "F-ordinal%d" % o0
        g = RE.gold(key, "replay3")
        kept = sorted(o for o, _n, _s in g.rows[0])
        assert kept[0] < RE.TILE and kept[-1] >= 2 * RE.TILE and any(o >= 3 for o in kept)
        assert set(o // RE.TILE for o in g.saved.tolist()) == {0, 1, 2}
        assert min(g.saved) < 3 <= max(g.saved)                                     # flags on both sides of the wrap
        want = RE.want_rows(g, 1, o0)[0]
        assert all(o >= o0 for _s, o in want) and (o0 < 2 ** 32 - 3 or any(o >> 32 for _s, o in want))
    first, n = RE.F_RANGE
    assert first % RE.TILE and (first + n) % RE.TILE and 2 * RE.TILE < first + n < RE.F_DB    # both ends inside a tile, three tiles touched
    assert len(RE.CASES["F-pool-cut-both-ends"].refs) == RE.F_DB
    g = RE.gold("F-pool-cut-both-ends", "replay3-res-h32")
    assert 0 in g.saved and max(g.saved) > RE.TILE


def test_f_lengths_on_both_sides_of_the_switch():
    ks = [k for k in RE.keys("F") if "nchar" in RE.CASES[k].meta]
    assert sorted(set(RE.CASES[k].meta["nchar"] for k in ks)) == [RE.WIDE_ABOVE, RE.WIDE_ABOVE + 1]
    assert sorted(set(len(RE.CASES[k].queries) for k in ks)) == [1, RE.F_NQ_MANY] and RE.F_NQ_MANY > 64
    case = RE.CASES["F-nchar%d-q1" % RE.WIDE_ABOVE]
    refs, probe = list(case.refs), RE.rows(case.queries)[0]
    assert len(refs) == RE.F_N and all(len(r) == RE.WIDE_ABOVE for r in refs)
    assert refs[17] == probe and set(refs[64]) == {ord("N")} and set(refs[65]) == {ord("-")}
    assert all(a != b for a, b in zip(refs[66], probe))
    assert RE.WIDE_ABOVE < 2 ** 16 and not case.meta["wide"] and RE.CASES["F-nchar%d-q1" % (RE.WIDE_ABOVE + 1)].meta["wide"]


# ---------------------------------------------------------------------------------------------------------------------------- C
def _c_expected_row(q, pi, ref, snap, acgt):
    """the six scores the oracle's loop gives a pair whose pre-score is cut at snap, from the oracle's own pieces: the untruncated scores of the pair
    (Query.allpairs) less what the cut takes from the consensus counters (score4 / score_acgt with and without maxdist)"""
    full = [int(x) for x in q.allpairs([ref])[0, pi]]
    score = O.score_acgt if acgt else O.score4
    u, c = score(ref, q.consensus, idx=q.idx_c), score(ref, q.consensus, maxdist=snap, idx=q.idx_c)
    if acgt:                                                            # src/nearest.c:462-469: matches, pairs, matches off idx_c, valid sites, mismatches on idx_c + idx_m, on idx
        lost_mis, lost_both = u[0] - c[0], u[1] - c[1]
        return (full[0] - (lost_both - lost_mis), full[1] - lost_both, full[2], full[3], full[4] - lost_mis, full[5]), c, u
    return tuple(full[i] - (u[i] - c[i]) for i in range(4)) + (full[4], full[5]), c, u      # src/nearest.c:497-500


@functools.lru_cache(maxsize=None)
def _c_report(key):
    """per plant of a case and per mode: cut_walk's answer, the oracle's cut and uncut consensus counters, the row the final heap must hold, and the
    counters of every wrong walk"""
    case = RE.CASES[key]
    refs, plants = list(case.refs), case.meta["plants"].get()
    W4 = RE.lane_split(case.meta["ncol"])[0]
    out = {}
    for acgt, regime in ((False, "replay3"), (True, "replay2-acgt")):
        q, pi = RE.query(key, regime), RE.probe_index(key, regime)
        for o, p in plants.items():
            cw = RE.cut_walk(q.consensus, q.idx_c, refs[o], p["snap"], acgt, W4)
            row, c, u = _c_expected_row(q, pi, refs[o], p["snap"], acgt)
            wrong = {w: RE.cut_walk(q.consensus, q.idx_c, refs[o], p["snap"], acgt, W4, wrong=w, every=q.seqs[pi]).counters for w in RE.CUT_WRONG}
            out[o, acgt] = (cw, tuple(c), tuple(u), row, wrong)
    return out


def test_c_geometries_snapshots_pools_and_regimes():
    assert {n: RE.lane_split(n)[1:] for n in RE.C_GEOMETRIES} == RE.C_GEOMETRIES
    assert [RE.C_GEOMETRIES[n][1] for n in sorted(RE.C_GEOMETRIES)] == [1, 2, 2, 3]                      # one word per lane | two, ragged | two, full | three, ragged
    assert 2048 == 64 * 32 and 2049 == 2048 + 1 and 4096 == 2 * 2048                                    # the last length of B = 1, the first of B = 2, the last of B = 2
    assert RE.lane_split(4097)[2] == 3 and 4200 % 32 == 8 and -(-4200 // 32) == RE.C_GEOMETRIES[4200][0]   # 4200: the last word holds eight sites, no padding word
    assert RE.C_GEOMETRIES[2049][0] - (-(-2049 // 32)) == 3                                             # 2049: three padding words, lane 33 holds nothing but them
    assert RE.C_POOLS == (RE.TILE, 2 * RE.TILE + 9) and RE.C_NBEST <= min(RE.C_POOLS) and RE.C_NBEST <= RE.MC_LIMIT
    cases = [RE.CASES[k] for k in RE.keys("C")]
    for n in RE.C_GEOMETRIES:
        mine = [c for c in cases if c.meta["ncol"] == n]
        assert set(s for c in mine for s in c.meta["snaps"]) == set(RE.C_SNAPS) and {"single"} < set(c.meta["kind"] for c in mine), n
        assert all((set(RE.C_RESIDENT) <= set(c.regimes)) == (n in (2049, 4200)) for c in mine)
    assert max(RE.C_SNAPS) > 32 and {1, 2, 3} < set(RE.C_SNAPS)
    assert set(c.pool for c in cases) == set(RE.C_POOLS) and {"single", "trim", "three", "two"} == set(c.meta["kind"] for c in cases)
    assert all(set(RE.C_PUSH) <= set(c.regimes) and len(c.refs) <= 3 * c.pool for c in cases)
    assert set(RE.C_PUSH) == {"replay3", "replay3-h8", "replay2", "replay2-acgt", "wide", "wide-acgt"}


@pytest.mark.parametrize("key", RE.keys("C"))
def test_c_every_plant_is_cut_where_it_is_named_and_keeps_its_cut_scores(key):
    case = RE.CASES[key]
    m = case.meta
    refs, plants, pool, snaps = list(case.refs), m["plants"].get(), case.pool, m["snaps"]
    ncol, window = m["ncol"], m["ncol"] - 2 * m["trim"]
    rep = _c_report(key)
    for acgt, regime in ((False, "replay3"), (True, "replay2-acgt")):
        q, pi, g = RE.query(key, regime), RE.probe_index(key, regime), RE.gold(key, regime)
        # ---- the query set: idx_c as the builder computed it, a proper subset of the window unless the probe is alone and untrimmed
        ic = RE.c_idx_c(case.queries, m["trim"])
        assert np.array_equal(q.idx_c, ic) and q.consensus[int(ic[0])] == RE.rows(case.queries)[0][int(ic[0])] and q.trim == m["trim"]
        assert 0 < len(q.idx_c) <= window and (len(q.idx_c) < window) == (m["kind"] in ("three", "two")) and (window < ncol) == (m["kind"] in ("three", "trim"))
        if m["kind"] == "three":
            assert not set(range(32 * RE.C_OUT_WORD, 32 * RE.C_OUT_WORD + 32)) & set(ic.tolist()) and len(q.idx_m) == 3 and len(q.idx) == 62
        # ---- the snapshots: the largest tolerance at the start of pools 1 and 2 is the one the plants are built for, and it has risen when they arrive
        for p, s in enumerate(snaps, start=1):
            before = O.search(q, refs[:p * pool], RE.names(p * pool), pool=pool, nbest=case.nbest, ambig_r=1.0)
            assert max(before.final_T) == before.final_T[pi] == s and all(n == case.nbest for n in before.heap_n)
            early = p * pool + 3
            after = O.search(q, refs[:early + 1], RE.names(early + 1), pool=pool, nbest=case.nbest, ambig_r=1.0)
            assert after.final_T[pi] == s + RE.C_BIG + 1 and early in after.saved
            if q.ntax > 1:                                              # the other queries' tolerances stay below: the plants are cut for them too and stop at their gates
                others = [t for i, t in enumerate(before.final_T) if i != pi]
                assert all(t < s for t in others) if (p == 2 or m["kind"] == "two") else all(t == s for t in others)
                assert [t for i, t in enumerate(g.final_T) if i != pi] == [t for i, t in enumerate(O.search(q, refs[:pool], RE.names(pool), pool=pool, nbest=case.nbest, ambig_r=1.0).final_T) if i != pi]
        assert g.final_T[pi] == snaps[-1] + RE.C_BIG + 1
        # ---- who enters: the lows, the two early plants, every plant -- and no decoy, each of which is cut with no match in front of the cut
        assert g.saved.tolist() == sorted(list(range(RE.C_NBEST)) + [p * pool + 3 for p in range(1, len(snaps) + 1)] + list(plants))
        for p, s in enumerate(snaps, start=1):
            for o in (p * pool + 2, p * pool + 4, min(len(refs), (p + 1) * pool) - 1):
                cw = RE.cut_walk(q.consensus, q.idx_c, refs[o], s, acgt)
                assert o not in plants and cw.cut and cw.counters[0 if not acgt else 1] == (0 if not acgt else s) and cw.col == int(ic[s - 1])
        final = RE.want_rows(g, q.ntax)
        assert sum(1 for _s, o in final[pi] if o < RE.C_NBEST) >= 2                  # lows are left: no plant was ever the worst kept entry
        for iq in range(q.ntax):
            assert iq == pi or not set(o for _s, o in final[iq]) & set(plants)
        # ---- every plant
        for o, p in plants.items():
            cw, c, u, row, _wrong = rep[o, acgt]
            s = p["snap"]
            assert o // pool == p["pool"] and s == snaps[p["pool"] - 1]
            assert cw.counters[:len(c)] == c, (key, p["name"], acgt)                  # the model's walk is the oracle's
            mis_u = u[0] if acgt else u[3] - u[0]
            assert cw.cut == (mis_u >= s)
            assert (row, o) in final[pi], (key, p["name"], acgt)                      # in the final heap, with the scores the cut leaves
            if "uncut-by-one" in p["want"]:
                assert not cw.cut and mis_u == s - 1 and c == u
                continue
            assert cw.cut and (c != u or cw.col == int(ic[-1])) and (c[0] if not acgt else c[1] - c[0]) >= RE.C_KEY0_MIN
            if not acgt:
                tags = RE.c_tags(cw, refs[o], case.queries[0], ic, s, ncol)
                assert p["want"] <= tags, (key, p["name"], p["want"] - tags)
                if "last-column" in tags:
                    assert c == u
                if "r-before" in tags:                                  # R over the consensus's A: a mismatch of the default walk, no pair at all under --acgt
                    assert rep[o, True][0].col > cw.col
    # pools of two tiles and nine: plants behind the early one in its tile and in both later tiles
    if pool > RE.TILE:
        for p in range(1, len(snaps) + 1):
            assert set((o - p * pool) // RE.TILE for o, x in plants.items() if x["pool"] == p) == {0, 1, 2}


@pytest.mark.parametrize("ncol", sorted(RE.C_GEOMETRIES))
def test_c_covers_every_position(ncol):
    seen, regimes = set(), set()
    for key in RE.keys("C"):
        case = RE.CASES[key]
        if case.meta["ncol"] != ncol:
            continue
        ic = RE.c_idx_c(case.queries, case.meta["trim"])
        refs = list(case.refs)
        for o, p in case.meta["plants"].get().items():
            cw = _c_report(key)[o, False][0]
            seen |= RE.c_tags(cw, refs[o], case.queries[0], ic, p["snap"], ncol) if cw.cut else {"uncut-by-one"}
        regimes |= set(case.regimes)
    req = RE.c_required_tags(ncol)
    assert req <= seen, sorted(req - seen)
    NW, B, lanes = RE.C_GEOMETRIES[ncol]
    assert ("pos-inner" in req) == (B == 3) and ("lane63" in req) == (lanes == 64) and ("pos-only" in seen) == (B == 1)
    assert "lane%d" % ((ncol - 1) // 32 // B) in seen                   # the last lane that holds a site
    assert set(RE.C_PUSH) <= regimes


@pytest.mark.parametrize("wrong", RE.CUT_WRONG)
@pytest.mark.parametrize("ncol", sorted(RE.C_GEOMETRIES))
def test_c_a_wrong_cut_does_not_pass(ncol, wrong):
    """stop one mismatch early, one late, count the whole word of the cut, lose the lanes in front at the lane of the cut, walk every column: in either mode some
    plant of every geometry has other counters than the oracle's, so its printed row would differ"""
    for acgt in (False, True):
        differ = []
        for key in RE.keys("C"):
            if RE.CASES[key].meta["ncol"] == ncol:
                differ += [RE.CASES[key].meta["plants"].get()[o]["name"] for (o, a), (_cw, c, _u, _row, w) in _c_report(key).items() if a == acgt and w[wrong][:len(c)] != c]
        assert differ, (ncol, wrong, acgt)
