"""The inputs of tests/ball_edges.py through the radius search on the MI355X (`pytest -m gpu`): stage 1, the gather of the columns of
query->idx by a pass of its own (ball_gather = 1) or inside stage 1 (2), the scan and the walk over the queries.  Every comparison is
np.array_equal on the whole cq->mindist against `oracle_lib.Query(..., is_ball=True).ball(refs, ambig_r=0.001)`; where a test also counts
the references that went on to the queries it holds uvaia_gpu_ball_asked against the model of ball_edges.  tests/test_ball_edges_cpu.py
shows which edge each input reaches."""
import numpy as np
import pytest

import ball_edges as BE
from uvaia_amd import capi

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("acgt", [False, True], ids=["default", "acgt"])
GATHER = pytest.mark.parametrize("gather", [1, 2], ids=["own-pass", "fused"])


def engine(q, gather):
    return capi.Engine.from_query(q, nbest=2, max_pool=BE.MAX_POOL, tuning={"ball_gather": gather})


def want_of(q, refs):
    return q.ball(refs, ambig_r=0.001)[0]                    # ambig_r ~ 0: no reference is filtered before scoring


def same(got, want, what):
    assert np.array_equal(got, want), (what, np.nonzero(np.asarray(got) != np.asarray(want))[0][:8].tolist(), np.asarray(got)[:8], want[:8])


# ---------------------------------------------------------------------------------------------------------------------------- A
@GATHER
@MODES
@pytest.mark.parametrize("name", BE.A_NAMES)
def test_a_number_and_placement_of_gathered_columns(name, acgt, gather):
    q, refs = BE.group_a(name, acgt)
    with engine(q, gather) as eng:
        same(eng.ball(refs, BE.A_RADIUS), want_of(q, refs), name)
        assert eng.ball_asked(reset=True) == BE.n_asked(q, refs, BE.A_RADIUS), name
        same(eng.ball(refs[:BE.TILE + 1], BE.A_RADIUS), want_of(q, refs)[:BE.TILE + 1], name)      # a shorter batch in the same buffers


# ---------------------------------------------------------------------------------------------------------------------------- B
@GATHER
@MODES
def test_b_query_tiles_and_the_first_query_below_the_limit(acgt, gather):
    for nq in BE.B_NQ:
        q, cases = BE.group_b(nq, acgt)
        refs = [c.ref for c in cases]
        want = want_of(q, refs)
        with engine(q, gather) as eng:
            got = eng.ball(refs, BE.B_RADIUS)
            for c, g, w in zip(cases, got, want):
                assert g == w, (nq, c.name, int(g), int(w))
            same(eng.ball(refs[::-1], BE.B_RADIUS), want[::-1], nq)      # other lanes, the same answers


# ---------------------------------------------------------------------------------------------------------------------------- C
@GATHER
@MODES
@pytest.mark.parametrize("name", list(BE.C_CASES))
def test_c_early_exit_and_padding_lanes(name, acgt, gather):
    q, refs = BE.group_c(name, acgt)
    want = want_of(q, refs)
    with engine(q, gather) as eng:
        for n in (BE.TILE, BE.TILE + 1, BE.TILE):                        # one full tile | one more lane and 63 padding lanes | again
            same(eng.ball(refs[:n], BE.C_RADIUS), want[:n], (name, n))
            assert eng.ball_asked(reset=True) == n
        same(eng.ball([refs[BE.C_LANE]], BE.C_RADIUS), want[BE.C_LANE:BE.C_LANE + 1], (name, "alone"))


# ---------------------------------------------------------------------------------------------------------------------------- D
@GATHER
@MODES
def test_d_stage_one_arithmetic(acgt, gather):
    for name in BE.D_SETS:
        eng = None
        try:
            for radius in BE.D_RADII:
                q, refs = BE.group_d(name, acgt, radius)                 # the same query set for every radius: one engine
                eng = eng or engine(q, gather)
                same(eng.ball(refs, radius), want_of(q, refs), (name, radius))
                assert eng.ball_asked(reset=True) == BE.n_asked(q, refs, radius), (name, radius)
        finally:
            if eng:
                eng.close()


# ---------------------------------------------------------------------------------------------------------------------------- E
@GATHER
@MODES
def test_e_survivor_lists_around_a_tile_in_reused_buffers(acgt, gather):
    q, refs, asks = BE.group_e(acgt)
    want = want_of(q, refs)
    R = BE.E_RADIUS

    def run_subset(eng, count, layout):
        sub = BE.e_subset(asks, count, layout)
        same(eng.ball([refs[i] for i in sub], R), want[sub], (count, layout))
        assert eng.ball_asked(reset=True) == count, (count, layout)

    with engine(q, gather) as eng:
        for layout in ("scattered", "one-tile"):
            for count in BE.E_ORDER:
                run_subset(eng, count, layout)
        eng.db_reserve(len(refs))
        eng.db_append(refs[:BE.E_FIRST_APPEND])
        same(eng.ball_resident(R), want[:BE.E_FIRST_APPEND], "resident 70")
        assert eng.ball_asked(reset=True) == asks[:BE.E_FIRST_APPEND].sum()
        eng.db_append(refs[BE.E_FIRST_APPEND:])                           # more than max_pool: the work arrays and the fused gather buffer grow
        assert eng.db_size() == len(refs)
        same(eng.ball_resident(R), want, "resident 1400")
        assert eng.ball_asked(reset=True) == asks.sum()
        run_subset(eng, 257, "scattered")                                 # the batch path after the resident one: unchanged
        run_subset(eng, 1, "one-tile")


# ---------------------------------------------------------------------------------------------------------------------------- F
@pytest.fixture(scope="module")
def f_tiles():
    """the interchange tiles of group F's references (the same in both modes), out of a default-mode context"""
    q, refs = BE.group_f(False)
    with engine(q, 2) as eng:
        eng.db_reserve(len(refs))
        eng.db_append(refs)
        return eng.db_export()[0]


@GATHER
@MODES
def test_f_ranges_and_batch_sizes(acgt, gather, f_tiles):
    q, refs = BE.group_f(acgt)
    assert refs == BE.group_f(False)[1]
    want = want_of(q, refs)
    asks = np.array([BE.stage(q, r, BE.F_RADIUS).asks for r in refs])
    R = BE.F_RADIUS
    with engine(q, gather) as eng:
        eng.db_reserve(BE.F_DB)
        eng.db_append(refs[:BE.F_DB])
        for first, n in BE.F_RANGES:
            same(eng.ball_resident(R, first, n), want[first:first + n], (first, n))
            assert eng.ball_asked(reset=True) == asks[first:first + n].sum(), (first, n)
        for n in BE.F_BATCHES:
            same(eng.ball(refs[:n], R), want[:n], ("text", n))
            assert eng.ball_asked(reset=True) == asks[:n].sum(), ("text", n)
            same(eng.ball_packed(f_tiles, n, R), want[:n], ("packed", n))     # the last tile's lanes past n hold further references
            assert eng.ball_asked(reset=True) == asks[:n].sum(), ("packed", n)
        assert eng.db_size() == BE.F_DB
        for first, n in ((BE.F_DB, 1), (0, BE.F_DB + 1), (150, 51)):          # uvaia_gpu_ball_resident: a range past the database
            with pytest.raises(capi.GpuError) as ei:
                eng.ball_resident(R, first, n)
            assert ei.value.code == -1
        with pytest.raises(capi.GpuError) as ei:                              # uvaia_gpu_ball: a batch above max_pool
            eng.ball(refs + refs[:1], R)
        assert ei.value.code == -6
        with pytest.raises(capi.GpuError) as ei:                              # uvaia_gpu_ball_packed: the same
            eng.ball_packed(np.concatenate([f_tiles, f_tiles[:1]]), BE.MAX_POOL + 1, R)
        assert ei.value.code == -6
        same(eng.ball_resident(R), want[:BE.F_DB], "after the refusals")
