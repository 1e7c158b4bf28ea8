"""The inputs of tests/replay_edges.py through the four replay kernels on the MI355X (`pytest -m gpu`), each under every regime of
launch_replay that has the edge (replay_edges.REGIMES: how the regime is selected).  Every comparison is equality with the oracle's search of
the same stream: the heaps (six scores and ordinal per slot, best first, via capi.finalise_heaps), the final tolerances and the entered
flags.  What is cheap to observe of the routing is asserted next to it: uvaia_gpu_scan_variant, the admissions and on-demand evaluations
of uvaia_gpu_replay_stats, and uvaia_gpu_replay_tiles_opened where replay3_kernel runs.  tests/test_replay_edges_cpu.py shows which edge
each input reaches."""
import numpy as np
import pytest

import replay_edges as RE
from uvaia_amd import capi

pytestmark = pytest.mark.gpu


def cases(group):
    runs = RE.runs(group)
    return pytest.mark.parametrize("key,regime", runs, ids=[RE.run_id(k, r) for k, r in runs])


def search(key, regime):
    """the case's stream through the regime's path; returns (heaps best first, tolerances, entered flags of the stream, the routing's facts)"""
    case, r = RE.CASES[key], RE.REGIMES[regime]
    q = RE.query(key, regime)
    refs = list(case.refs)
    o0 = case.meta.get("ordinal0", 0)
    tuning = dict(r.tuning)
    if r.path == "resident":
        tuning["subslice_refs"] = max(RE.TILE, len(refs))                    # one slice per run
    with capi.Engine.from_query(q, nbest=case.nbest, max_pool=case.pool if r.path == "push" else len(refs), tuning=tuning or None) as eng:
        if r.path == "push":
            ent = np.concatenate([eng.push(refs[a:a + case.pool], ordinal0=o0 + a) for a in range(0, len(refs), case.pool)])
        else:
            eng.db_reserve(len(refs))
            eng.db_append(refs)
            eng.reset()
            if eng.scan_variant() == 2:
                eng.db_rederive()
            if "range" in case.meta:
                first, n = case.meta["range"]
                eng.search_resident_pool(first, n, o0)
                eng.sync()
                ent = eng.entered_flags()
                assert not ent[:first].any() and not ent[first + n:].any()
                ent = ent[first:first + n]
            else:
                ent = eng.search_resident(case.pool, ordinal0=o0)
                eng.sync()
        n, T, sc, od = eng.drain()
        admitted, demanded, dense = eng.replay_stats()
        facts = {"scan": eng.scan_variant(), "admitted": admitted, "demanded": demanded, "dense": dense, "opened": eng.replay_tiles_opened()}
    return capi.finalise_heaps(n, sc, od), [int(t) for t in T], ent, facts


def check(key, regime):
    case, r = RE.CASES[key], RE.REGIMES[regime]
    q, g = RE.query(key, regime), RE.gold(key, regime)
    rows, T, ent, facts = search(key, regime)
    want = RE.want_rows(g, q.ntax, case.meta.get("ordinal0", 0))
    for iq in range(q.ntax):
        assert rows[iq] == want[iq], (RE.run_id(key, regime), "query", iq, "probe" if iq == RE.probe_index(key, regime) else "filler")
    assert T == [int(t) for t in g.final_T]
    assert np.nonzero(ent)[0].tolist() == g.saved.tolist()
    # ---- the routing
    kernel = r.kernel or ("replay" if case.meta["wide"] else "replay2" if (r.acgt or q.ntax > 32) else "replay3")
    assert facts["scan"] == (-1 if kernel == "replay" else 0 if q.ntax <= 32 else 2), facts
    if kernel == "replay3":
        assert facts["opened"] > 0 and (case.group in "SC" or facts["demanded"] < facts["admitted"]), facts     # (S, C: slow pairs are evaluated on demand)
    elif kernel == "replay":
        assert facts["opened"] == 0 and facts["admitted"] == 0 and facts["demanded"] == 0, facts      # replay_kernel keeps no statistics
    else:
        assert facts["opened"] == 0 and facts["demanded"] >= facts["admitted"] > 0, facts
    return facts


@cases("R")
def test_r_rounds_of_tile_bounds_and_the_ring(key, regime):
    """plants at lanes 0 and 63 of the first and last tile of rounds 0, 3, 4, 8, 9, 12, 13, 15, 16, 17, 31, 32 and in the partial last tile, far
    references elsewhere: bounds read from the wrong round or slot skip a plant's tile"""
    facts = check(key, regime)
    nt = RE.CASES[key].meta["n_tiles"]
    if RE.REGIMES[regime].kernel == "replay3" and nt >= RE.TILE:
        assert facts["opened"] < nt * len(RE.CASES[key].queries) / 2, facts           # whole tiles are skipped (test_replay_edges_cpu: < 5 % hold an admission)


@cases("G")
def test_g_a_skipped_tile_becomes_needed(key, regime):
    """the tolerance jumps from 3 to 10 in tile u; tile x, passed over by the bounds before, must be opened in stream order: between tiles in flight
    (regroup), behind them, in the same half, at the head of the next half, in the next round; and the mirror, tiles in flight under a tolerance that fell"""
    check(key, regime)


@cases("H")
def test_h_heap_layout_among_full_ties(key, regime):
    """3 x nbest references of 13 score vectors: which ordinal is evicted among entries equal on all six keys is the layout of src/min_heap.c"""
    check(key, regime)


@cases("K")
def test_k_the_key_ladder(key, regime):
    """B ties the worst kept entry A on keys 0 .. j - 1 and differs by one at key j, in both directions; equal on all six; ahead with m == T"""
    check(key, regime)


@cases("T")
def test_t_tolerances_against_the_thresholds_of_the_bounds(key, regime):
    """T - 1 at every entry of TB8_THR and one past it: T - 1 mismatches enter, T mismatches do not, the next threshold's count is refused by the gate"""
    check(key, regime)


@cases("S")
def test_s_slow_pairs(key, regime):
    """ambiguity-word lists of 0, 1, 10, 11 and 12 words on either side, shared words, pairs cut at the batch snapshot next to uncut ones"""
    facts = check(key, regime)
    if RE.REGIMES[regime].kernel in ("replay2", "replay3"):
        assert (facts["dense"] > 0) == RE.CASES[key].meta["dense"], facts


@cases("C")
def test_c_the_cut_of_the_consensus_prescore(key, regime):
    """pre-scores cut at snapshots of 1, 2, 3 and 40 at 2048, 2049, 4096 and 4200 columns: the cut at bit 0 and bit 31, in the first, an inner and the last word
    of a lane's range, in lane 0, lane 63 and the last lane that holds a site, at the last column of idx_c, behind N, R and substitutions outside idx_c; every
    cut pair stays in the final heap, so a cut one site off is a wrong row"""
    facts = check(key, regime)
    if RE.REGIMES[regime].kernel in ("replay2", "replay3"):
        assert facts["demanded"] > 0, facts                                                           # the on-demand walk ran


@cases("F")
def test_f_range_ends(key, regime):
    """ordinals whose low word wraps inside a tile and whose high word is set; a pool cut inside a tile at both ends; 49 000 and 49 001 columns"""
    check(key, regime)
