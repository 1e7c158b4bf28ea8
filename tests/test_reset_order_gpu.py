"""uvaia_gpu_reset is one kernel launch that the host does not wait for, and uvaia_gpu_db_rederive issues its first chunk without
fences when nothing is in flight: the order comes from the streams.  70 queries (column-compressed scan on request, the rebuild does
something) and 4 queries (packed-plane scan, the replay kernels on a stream of their own) x 300 references x 2 300 columns, pools
of 100 references, against the oracle."""
import functools

import numpy as np
import pytest

import fixtures as F
import oracle_lib as O
from uvaia_amd import capi

pytestmark = pytest.mark.gpu

NREF, NCHAR, POOL, NBEST = 300, 2300, 100, 6


@functools.lru_cache(maxsize=None)
def _case(nq, acgt):
    """inputs and, computed once, the oracle over the references and over the references offered twice in a row"""
    refs, root, cols = F.synth_alignment(NREF, NCHAR, seed=61)
    qs, _, _ = F.synth_alignment(nq, NCHAR, seed=161, root=root, poly_cols=cols)
    q = O.Query(qs, ["q%d" % i for i in range(len(qs))], acgt=acgt)
    names = ["r%d" % i for i in range(NREF)]
    once = O.search(q, refs, names, pool=POOL, nbest=NBEST, ambig_r=1.0)
    twice = O.search(q, refs + refs, names + ["s%d" % i for i in range(NREF)], pool=POOL, nbest=NBEST, ambig_r=1.0)
    return q, refs, once, twice


def _rows(gold):
    return [[(tuple(s), o) for o, _, s in rows] for rows in gold.rows]


def _engine(q, refs):
    eng = capi.Engine.from_query(q, nbest=NBEST, max_pool=128, tuning={"scan": "compressed"} if q.ntax > 32 else None)
    eng.db_reserve(len(refs))
    eng.db_append(refs[:130])
    eng.db_append(refs[130:])
    return eng


CASES = [(70, False), (70, True), (4, False)]


@pytest.mark.parametrize("nq,acgt", CASES)
def test_reset_then_drain_at_once(nq, acgt):
    q, refs, once, _ = _case(nq, acgt)
    with _engine(q, refs) as eng:
        eng.search_resident(POOL, want_entered=False)      # heaps, tolerances and flags hold something
        eng.reset()
        n, T, sc, od = eng.drain()
        assert not n.any() and not sc.any() and not od.any()
        assert list(T) == [q.nchar] * q.ntax
        assert not eng.entered_flags().any()


@pytest.mark.parametrize("nq,acgt", CASES)
def test_reset_rederive_search_without_a_wait_between_them_twice(nq, acgt):
    q, refs, once, _ = _case(nq, acgt)
    with _engine(q, refs) as eng:
        for _ in range(2):                                 # the second round queues behind the first one's scans and replays
            eng.reset()
            eng.db_rederive()
            eng.search_resident(POOL, want_entered=False)
        n, T, sc, od = eng.drain()
        assert capi.finalise_heaps(n, sc, od) == _rows(once)
        assert list(T) == once.final_T
        assert list(np.nonzero(eng.entered_flags())[0]) == list(once.saved)
        eng.reset()                                        # and with the result of every round looked at
        eng.db_rederive()
        ent = eng.search_resident(POOL)
        n, T, sc, od = eng.drain()
        assert capi.finalise_heaps(n, sc, od) == _rows(once) and list(T) == once.final_T
        assert list(np.nonzero(ent)[0]) == list(once.saved)


@pytest.mark.parametrize("nq,acgt", CASES)
def test_two_searches_without_a_reset_leave_the_flags_of_the_second(nq, acgt):
    """the references offered a second time (ordinals 300 ..) to the heaps the first search left = the oracle over the stream twice in a
    row; the entered flags are those of its second half only -- the search clears them itself where no reset has"""
    q, refs, once, twice = _case(nq, acgt)
    with _engine(q, refs) as eng:
        eng.reset()
        ent1 = eng.search_resident(POOL)
        assert list(np.nonzero(ent1)[0]) == list(once.saved)
        eng.search_resident(POOL, ordinal0=NREF, want_entered=False)
        n, T, sc, od = eng.drain()
        assert capi.finalise_heaps(n, sc, od) == _rows(twice) and list(T) == twice.final_T
        assert list(np.nonzero(eng.entered_flags())[0] + NREF) == [o for o in twice.saved if o >= NREF]
