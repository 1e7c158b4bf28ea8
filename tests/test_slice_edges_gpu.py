"""The slice plan of the resident search on the MI355X (`pytest -m gpu`): what plan_subslices (host_resident.inc) decides, read through
uvaia_gpu_search_plan, and the searches and rebuilds that run along it (run_subslices, uvaia_gpu_db_rederive).

  1. invariants of the plan over a grid of ranges and pools, for contexts on both sides of every query-tile threshold (host arithmetic only);
  2. the inputs of tests/slice_edges.py, one db_append_block + search_resident each, against the oracle -- after an assertion that the plan has the
     shape the case is built for, so that a retune that moves a threshold fails here and the case is re-aimed instead of going quiet;
  3. tuning.scan_streams, tuning.rederive_streams and tuning.serial over a shape with six times as many slices as counter buffers: every run equals
     the oracle, a rebuild changes nothing;
  4. a rebuild whose chunks share tiles (max_pool 100): the derived planes are the ones the appends wrote, byte for byte."""
import types

import numpy as np
import pytest

import slice_edges as S
from uvaia_amd import capi

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------- 1. invariants of the plan
FIRSTS = (0, 1, 64, 100)
LENGTHS = (1, 63, 64, 65, 1000, 62757, 163877, 8 * 65536 - 1, 8 * 65536, 12 * 65536, 12 * 65536 + 1, 2000000)
POOLS = (1, 63, 64, 100, 65536, 300000, None)              # None: the whole range
QUERY_COUNTS = (1, 48, 49, 256, 257, 512, 513, 992, 993)    # both sides of 4, 17, 33 and 63 tiles of 16 queries


def _contexts():
    out = []
    for nq in QUERY_COUNTS:
        for cons in (True, False):
            for acgt in (False, True):
                out.append((nq, cons, acgt, {}, None))
    for nq in (1, 49, 513):
        for cons in (True, False):
            for sub in (0, 64, 448):
                for streams in (0, 150, 199):
                    if sub or streams:
                        out.append((nq, cons, nq == 49, dict(({"subslice_refs": sub} if sub else {}), **({"scan_streams": streams} if streams else {})), None))
    out.append((993, True, False, {}, (64, 320)))             # narrowed to 16 query tiles: below HEAD_TAIL_NQT with 993 queries open
    out.append((993, False, False, {}, (64, 128)))
    return out


def _context_id(ctx):
    nq, cons, acgt, tuning, active = ctx
    return "q%d-%s-%s%s%s" % (nq, "cons" if cons else "nocons", "acgt" if acgt else "iupac", "".join("-%s%d" % (k[:3], v) for k, v in sorted(tuning.items())),
                              "-active%d_%d" % active if active else "")


def plan_query(nq, cons, acgt):
    """a prepared query set of NCHAR columns; without `cons` the constant-and-complete columns are handed over as constant ones with a missing
    site (the counters do not depend on the split), so that n_idx_c == 0 whatever the number of queries"""
    Q, _ = S.make_queries(nq, True)
    q = S.O.Query([r.tobytes() for r in Q], ["q%d" % i for i in range(nq)], acgt=acgt, ambig_q=1.0)
    assert len(q.idx_c) > 0
    if cons:
        return q
    return types.SimpleNamespace(seqs=q.seqs, consensus=q.consensus, idx_c=np.zeros(0, dtype=np.int64), idx_m=np.sort(np.concatenate([q.idx_c, q.idx_m])),
                                 idx=q.idx, trim=q.trim, acgt=q.acgt, ntax=q.ntax)


def check_plan(sf, sn, ps, first, n, pool, cons, max_pool, what):
    sf, sn = sf.astype(np.int64), sn.astype(np.int64)
    assert len(sf) >= 1 and sf[0] == first and sf[-1] + sn[-1] == first + n, what
    assert np.array_equal(sf[1:], sf[:-1] + sn[:-1]), what                       # in order, no gap, no overlap
    assert sn.min() >= 1, what
    if cons:
        assert np.array_equal((sf - first) // pool, (sf + sn - 1 - first) // pool), what          # no slice crosses first + k * pool
        assert np.array_equal(ps != 0, (sf - first) % pool == 0), what
        assert sn.max() <= max_pool, what                                        # uvaia_gpu_slice_scan refuses a longer one
    else:
        assert ps[0] == 1 and not ps[1:].any(), what


@pytest.mark.parametrize("ctx", _contexts(), ids=_context_id)
def test_every_plan_tiles_its_range_and_marks_the_pools(ctx):
    nq, cons, acgt, tuning, active = ctx
    max_pool = 2000000 if nq <= 49 else 300000
    with capi.Engine.from_query(plan_query(nq, cons, acgt), nbest=S.NBEST, max_pool=max_pool, tuning=tuning) as eng:
        if active:
            eng.set_active_queries(*active)
        for bad in (0, max_pool + 1):
            with pytest.raises(capi.GpuError) as ei:
                eng.search_plan(0, 1000, bad)
            assert ei.value.code == -1                       # UVAIA_GPU_EINVAL, as uvaia_gpu_search_resident
        asked = 0
        for first in FIRSTS:
            for n in LENGTHS:
                for pool in sorted(set(n if p is None else p for p in POOLS)):
                    if pool > max_pool:
                        continue
                    sf, sn, ps = eng.search_plan(first, n, pool)
                    check_plan(sf, sn, ps, first, n, pool, cons, max_pool, (_context_id(ctx), first, n, pool))
                    asked += 1
        assert asked >= len(FIRSTS) * len(LENGTHS) * 5
        assert eng.db_size() == 0                            # nothing was loaded: the plan is arithmetic on the context alone


def test_the_plan_of_a_narrowed_context_is_the_plan_of_its_active_tiles():
    """993 queries open, 256 of them active: the head / middle / tail layout, which 63 query tiles never get"""
    with capi.Engine.from_query(plan_query(993, True, False), nbest=S.NBEST, max_pool=1000000) as eng:
        whole = eng.search_plan(0, 786469, 786469)
        eng.set_active_queries(64, 320)
        part = eng.search_plan(0, 786469, 786469)
    assert int(whole[1].max()) < S.HEAD and len(whole[1]) > len(part[1])
    assert int(part[1][0]) == S.HEAD and int(part[1][-1]) == S.TAIL and S.PRE not in [int(x) for x in part[1]]
    assert [tuple(int(v) for v in s[:2]) + (bool(s[2]),) for s in zip(*part)] == S.plan(0, 786469, 786469, 993, 1, False, active=(64, 320))


# ---------------------------------------------------------------------------------------------------------------- 2. searches at the branch points
def check_search(eng, gold, pool, what):
    ent = eng.search_resident(pool)
    n, T, sc, od = eng.drain()
    assert list(np.nonzero(ent)[0]) == list(gold.saved), what
    assert capi.finalise_heaps(n, sc, od) == S.want_rows(gold), what
    assert list(T) == gold.final_T, what
    return ent


@pytest.mark.parametrize("key", list(S.CASES))
@pytest.mark.parametrize("acgt", [False, True], ids=["iupac", "acgt"])
def test_search_at_a_branch_point_of_the_planner(key, acgt):
    c, pool = S.CASES[key], S.case_pool(key)
    q, gold = S.query(key, acgt), S.gold(key, acgt)
    with capi.Engine.from_query(q, nbest=S.NBEST, max_pool=pool) as eng:
        # the plan the case is built for: the slice count, which slices are exactly 65 536 or 131 072 and which are shorter or longer
        sf, sn, ps = eng.search_plan(0, c.n, pool)
        lengths = tuple(int(x) for x in sn)
        assert len(lengths) == len(c.lengths), (key, lengths)
        assert [x == S.HEAD for x in lengths] == [x == S.HEAD for x in c.lengths], (key, lengths)
        assert [x == S.PRE for x in lengths] == [x == S.PRE for x in c.lengths], (key, lengths)
        assert lengths == c.lengths, (key, lengths)
        got = [(int(a), int(b), bool(p)) for a, b, p in zip(sf, sn, ps)]
        assert got == S.case_plan(key, acgt, len(q.idx_c)), key               # the boundaries the pairs of identical references sit at
        assert eng.scan_variant() == (0 if c.nq <= S.PACKED_NQ else 2)
        eng.db_reserve(c.n)
        eng.db_append_block(S.refs(key))
        ent = check_search(eng, gold, pool, (key, acgt))
        for f, n, _ in got:                                  # no slice went by without an admission
            if n > S.WINDOW:
                assert ent[f:f + n].any(), (key, f, n)
        for b in S.boundaries(key):
            assert ent[b - 1] and ent[b], (key, b)


# ---------------------------------------------------------------------------------------------------------------- 3. the schedule knobs
SETTINGS = [{}] + [{"scan_streams": v} for v in (1, 2, 3, 150, 199)] + [{"rederive_streams": v} for v in (1, 2, 3)] + [{"serial": 1}]


def open_with_slices(q, nbest, max_pool, tuning, n, pool, at_least):
    """a context whose plan for [0, n) in batches of pool has `at_least` slices: without tuning.subslice_refs where that holds, with slices of two
    tiles otherwise"""
    eng = capi.Engine.from_query(q, nbest=nbest, max_pool=max_pool, tuning=tuning)
    if len(eng.search_plan(0, n, pool)[0]) >= at_least:
        return eng
    eng.close()
    eng = capi.Engine.from_query(q, nbest=nbest, max_pool=max_pool, tuning=dict(tuning, subslice_refs=128))
    assert len(eng.search_plan(0, n, pool)[0]) >= at_least
    return eng


@pytest.mark.parametrize("acgt", [False, True], ids=["iupac", "acgt"])
@pytest.mark.parametrize("scan", ["packed", "compressed"])
def test_the_schedule_knobs_change_no_result(scan, acgt):
    q, refs = S.knob_inputs(acgt)
    gold = S.knob_gold(acgt)
    assert len(q.idx_c) > 0
    n_tiles = (S.KNOB_NREF + 63) // 64
    first_derived = None
    for setting in SETTINGS:
        what = (scan, acgt, setting)
        with open_with_slices(q, S.KNOB_NBEST, 256, dict(setting, scan=scan), S.KNOB_NREF, S.KNOB_POOL, S.NBUF + 1) as eng:
            assert eng.scan_variant() == (2 if scan == "compressed" else 0)
            sf, sn, ps = eng.search_plan(0, S.KNOB_NREF, S.KNOB_POOL)
            assert len(sn) >= 20 and not (sf % 64).any(), what                   # whole tiles; every counter buffer is used five times and more
            eng.db_reserve(S.KNOB_NREF)
            eng.db_append(refs[:S.KNOB_CUT])
            eng.db_append(refs[S.KNOB_CUT:])
            appended = eng.db_derived(n_tiles) if scan == "compressed" else None
            check_search(eng, gold, S.KNOB_POOL, what + ("after the appends",))
            for again in (1, 2):                                                 # a rebuild and a search, twice on the same context
                eng.reset()
                eng.db_rederive()
                check_search(eng, gold, S.KNOB_POOL, what + ("after rebuild %d" % again,))
            if scan == "compressed":
                rebuilt = eng.db_derived(n_tiles)
                first_derived = first_derived or appended
                for which, a, b, d in zip(("e", "grp", "poly", "tot"), first_derived, appended, rebuilt):
                    assert np.array_equal(a, b), what + (which, "appended")
                    assert np.array_equal(a, d), what + (which, "rebuilt")
    if scan == "compressed":
        assert first_derived[0].any() and first_derived[3].any()


# ---------------------------------------------------------------------------------------------------------------- 4. rebuild chunks that share tiles
@pytest.mark.parametrize("acgt", [False, True], ids=["iupac", "acgt"])
def test_rebuild_chunks_that_share_tiles(acgt):
    q, refs = S.knob_inputs(acgt)
    refs = refs[:S.CHUNK_NREF]
    gold = S.knob_gold(acgt, S.CHUNK_NREF, S.CHUNK_POOL)
    assert len(q.idx_c) > 0
    n_tiles = (S.CHUNK_NREF + 63) // 64
    first = None
    for streams in (0, 1, 3):
        with capi.Engine.from_query(q, nbest=S.KNOB_NBEST, max_pool=S.CHUNK_POOL, tuning=dict({"scan": "compressed"}, **({"rederive_streams": streams} if streams else {}))) as eng:
            assert eng.scan_variant() == 2
            sf, sn, ps = eng.search_plan(0, S.CHUNK_NREF, S.CHUNK_POOL)          # the plan the rebuild follows: pool = max_pool
            assert len(sf) == 10 and int(np.count_nonzero(sf % 64)) == 9 and ps.all()
            eng.db_reserve(S.CHUNK_NREF)
            eng.db_append(refs[:S.CHUNK_CUT])
            eng.db_append(refs[S.CHUNK_CUT:])
            appended = eng.db_derived(n_tiles)
            check_search(eng, gold, S.CHUNK_POOL, (acgt, streams, "after the appends"))
            eng.reset()
            eng.db_rederive()
            rebuilt = eng.db_derived(n_tiles)
            check_search(eng, gold, S.CHUNK_POOL, (acgt, streams, "after the rebuild"))
            eng.reset()
            eng.db_rederive()                                                    # searched while the chunks are still in flight
            check_search(eng, gold, S.CHUNK_POOL, (acgt, streams, "behind the rebuild"))
        first = first or appended
        for which, a, b, d in zip(("e", "grp", "poly", "tot"), first, appended, rebuilt):
            assert np.array_equal(a, b), (acgt, streams, which, "appended")
            assert np.array_equal(a, d), (acgt, streams, which, "rebuilt")
    assert first[0].any() and first[3].any()
