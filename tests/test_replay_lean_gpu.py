"""replay2_lean_kernel -- the replay of a large query set in default mode -- against the CPU oracle at the edges of its regime (`pytest -m gpu`).

The engine launches that kernel when the query set has no constant-and-complete column, the query's planes are not cached in LDS (256
queries and more), the resident search requests two candidates ahead (more than 64 queries) and the heaps hold at most 127 entries; every
other case keeps replay2_kernel.  All cases here: 256 generator queries x 3 000 generator references x 2 000 columns through
db_append -> reset -> db_rederive -> search_resident, heaps (six scores and ordinal per slot, best first), final tolerances and dump flags
compared with the oracle's (src/nearest.c:288-306,479-510).  What each stream is for was checked with the oracle before the case was
written, and the checks that are cheap are asserted again below.
"""
import numpy as np
import pytest

import oracle_lib as O
from uvaia_amd import capi, hostlib

pytestmark = pytest.mark.gpu

QUERY_INDEX0 = 1 << 40          # as bench.py: queries and references come from disjoint sequence numbers of one generator
NQ, N_REF, NCHAR = 256, 3000, 2000
SLICE = 704                     # tuning.subslice_refs: the search lays four near-equal slices over the 3 000 references, whole tiles each ...
CUT = 768                       # ... at 0, 768, 1 536 and 2 304; the last one is 696 references, its last tile holds 56


def _names(n, p="r"):
    return ["%s%d" % (p, i) for i in range(n)]


def _want(gold, ntax):
    return [[(tuple(s), o) for o, _, s in gold.rows[iq]] for iq in range(ntax)]


class _Data:
    def __init__(self):
        self.gen = hostlib.Synth(NCHAR, seed=20241008, preset=0)
        self.qs, _ = self.gen.generate_bytes(QUERY_INDEX0, NQ)
        self.qn = _names(NQ, "query_")
        self.refs, _ = self.gen.generate_bytes(0, N_REF)
        self.oq = O.Query(self.qs, self.qn)
        self.pq = hostlib.PreparedQuery(self.qs, self.qn)
        assert self.pq.ntax == self.oq.ntax == NQ and len(self.pq.idx_c) == 0      # no consensus pre-score: CONS = false
        self._gold = {}

    def gold(self, nbest, pool=N_REF):
        """the oracle's answer to the plain stream, computed once per (nbest, pool) and not changed afterwards"""
        if (nbest, pool) not in self._gold:
            self._gold[(nbest, pool)] = O.search(self.oq, self.refs, _names(N_REF), pool=pool, nbest=nbest, ambig_r=0.5)
        return self._gold[(nbest, pool)]


@pytest.fixture(scope="module")
def data():
    return _Data()


def _search(eng, refs, pool, resets=True, ordinal0=0):
    if resets:
        eng.db_reserve(len(refs))
        eng.db_append(refs)
        eng.reset()
    eng.db_rederive()
    ent = eng.search_resident(pool, ordinal0=ordinal0)
    eng.sync()
    n, T, sc, od = eng.drain()
    return capi.finalise_heaps(n, sc, od), list(T), ent


def _check(got, gold, ntax=NQ):
    rows, T, ent = got
    assert rows == _want(gold, ntax)
    assert T == list(gold.final_T)
    assert list(np.nonzero(ent)[0]) == list(gold.saved)


@pytest.mark.parametrize("nbest", [3, 127, 128])
def test_several_slices_with_a_partial_last_tile(data, nbest):
    """(a), (b): four slices, the last one shorter with a partial last tile; heaps of 3 (full after three references: nearly
    every admission replaces the root), of 127 (the largest with a lane per inner node: the lean kernel's limit) and of 128 (one more:
    replay2_kernel with the level-by-level root replacement, which must still agree)."""
    gold = data.gold(nbest)
    assert all(len(r) == nbest for r in gold.rows)                          # the heaps fill, so root replacement runs for every query
    with data.pq.open_engine(nbest=nbest, max_pool=N_REF, tuning={"subslice_refs": SLICE}) as eng:
        assert eng.scan_variant() == 2
        got = _search(eng, data.refs, N_REF)
        assert eng.scan_stats()[1] == 4                                     # one scan launch per slice
        admitted, demanded, _dense = eng.replay_stats(reset=True)
    _check(got, gold)
    assert admitted >= NQ * nbest and demanded >= admitted


def test_far_references_first_then_close_ones(data):
    """(c): the first 200 references carry another base in every seventh column (some 280 mismatches more than the others), heaps of 100: they fill
    with far references, the tolerances start near 290, fall as close references displace the far ones and rise again whenever a new
    worst kept entry has more mismatches than the one before -- in every later slice for dozens of queries, which is when a tile the
    walk had passed over becomes needed while later ones are in flight."""
    rot = bytes.maketrans(b"ACGT", b"CGTA")

    def far(s):
        b = bytearray(s)
        b[::7] = bytes(b[::7]).translate(rot)
        return bytes(b)

    refs = [far(r) for r in data.refs[:200]] + data.refs[200:]
    gold = O.search(data.oq, refs, _names(N_REF), pool=N_REF, nbest=100, ambig_r=0.5)
    # what the case is for: between the ends of the second and the third slice some query's tolerance rises (no consensus columns, so a
    # search of a prefix leaves the state the whole search has at that point)
    t2 = np.array(O.search(data.oq, refs[:2 * CUT], _names(2 * CUT), pool=2 * CUT, nbest=100, ambig_r=0.5).final_T)
    t3 = np.array(O.search(data.oq, refs[:3 * CUT], _names(3 * CUT), pool=3 * CUT, nbest=100, ambig_r=0.5).final_T)
    assert (t3 > t2).any() and (t3 < t2).any()
    assert (gold.saved < 200).any()                                          # far references entered while the heaps filled
    with data.pq.open_engine(nbest=100, max_pool=N_REF, tuning={"subslice_refs": SLICE}) as eng:
        _check(_search(eng, refs, N_REF), gold)


def test_a_pool_inside_the_database_cuts_tiles(data):
    """(d): the pool of references 1 000 .. 1 999 of the 3 000 resident ones, in three slices of 384, 384 and 232: every slice begins at lane
    40 of a tile, the last one ends at lane 16 of one.  Its answer is the oracle's over those thousand references alone; the dump flags
    sit at their places in the database."""
    first, n = 1000, 1000
    gold = O.search(data.oq, data.refs[first:first + n], _names(n), pool=n, nbest=20, ambig_r=0.5)
    with data.pq.open_engine(nbest=20, max_pool=N_REF, tuning={"subslice_refs": 320}) as eng:
        eng.db_reserve(N_REF)
        eng.db_append(data.refs)
        eng.reset()
        eng.db_rederive()
        eng.search_resident_pool(first, n, 0)
        eng.sync()
        nn, T, sc, od = eng.drain()
        ent = eng.entered_flags()
    assert capi.finalise_heaps(nn, sc, od) == _want(gold, NQ) and list(T) == list(gold.final_T)
    assert list(np.nonzero(ent)[0] - first) == list(gold.saved)


def test_two_searches_without_a_reset_between(data):
    """(e): the second search starts from the heaps, counts and tolerances the first one left in memory and numbers its references behind
    the first one's: together they are one search of the stream sent twice."""
    gold = O.search(data.oq, data.refs + data.refs, _names(2 * N_REF), pool=N_REF, nbest=20, ambig_r=0.5)
    first = data.gold(20)
    assert list(gold.final_T) != list(first.final_T) and (gold.saved >= N_REF).any()     # the second pass admits and moves tolerances
    with data.pq.open_engine(nbest=20, max_pool=N_REF, tuning={"subslice_refs": SLICE}) as eng:
        _check(_search(eng, data.refs, N_REF), first)
        rows, T, ent = _search(eng, data.refs, N_REF, resets=False, ordinal0=N_REF)
    assert rows == _want(gold, NQ) and T == list(gold.final_T)
    assert list(np.nonzero(ent)[0] + N_REF) == [int(o) for o in gold.saved if o >= N_REF]   # the flags of the second search only
