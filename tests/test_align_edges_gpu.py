"""The inputs of tests/align_edges.py through wfa_align_kernel on the MI355X (`pytest -m gpu`): for every query of every pool the score and
the aligned row equal the oracle's byte for byte, the pool takes one pass, and the cells the kernel counts are the cells the oracle counts
(a wavefront with other limits that still ends on the same row does not pass).  tests/test_align_edges_cpu.py shows which edge of the
kernel each input reaches."""
import functools

import numpy as np
import pytest

import align_edges as AE
import oracle_lib as O
from uvaia_amd import align

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _gotoh(ref, q, pen):
    return O.gotoh_score(ref, q, pen)


def run_pool(pool, seqs=None):
    """the pool through one aligner against the oracle; returns (scores, rows) of the device"""
    seqs = list(pool.seqs if seqs is None else seqs)
    want = [AE.expected(pool.ref, q, pool.opts) for q in seqs]
    opts = dict(workspace_bytes=AE.WORKSPACE)
    opts.update(pool.opts)
    with align.Aligner(pool.ref, **opts) as al:
        score, rows = al.align(seqs)
        st = al.stats()
    for i, (q, (w_score, w_row, _, _, _)) in enumerate(zip(seqs, want)):
        assert score[i] == w_score, (pool.name, i, len(q), int(score[i]), w_score)
        assert rows[i].tobytes() == w_row, (pool.name, i, len(q))
    assert st["passes"] == 1, (pool.name, st)
    assert st["cells"] == sum(w[2] for w in want), (pool.name, st["cells"], sum(w[2] for w in want))
    if AE.is_complete(pool.opts):                       # the optimum itself, without the restated wavefronts in between
        pen = (0,) + AE.penalties_of(pool.opts)
        for i, q in enumerate(seqs):
            if len(pool.ref) * len(q) <= AE.GOTOH_CELLS:
                assert score[i] == _gotoh(pool.ref, q, pen), (pool.name, i, len(q))
    return score, rows


def test_a_offsets_around_16_bits():
    for pool in AE.group_a():
        run_pool(pool)


@pytest.mark.parametrize("setting", AE.B_SETTINGS, ids=lambda s: "-".join(str(v) for v in s.values()))
def test_b_widths_around_the_lds_ring_and_the_reduction(setting):
    for pool in AE.group_b(setting):
        run_pool(pool)


def test_b_end_diagonal_outside_the_first_reduced_wavefronts():
    for pool in AE.group_b_outside():
        run_pool(pool)


@pytest.mark.parametrize("name", AE.C_NAMES)
def test_c_penalties(name):
    for pool in AE.group_c(name):
        run_pool(pool)


def test_d_extension_runs_in_both_pool_orders():
    (pool,), _ = AE.group_d()
    s1, r1 = run_pool(pool)
    s2, r2 = run_pool(pool, pool.seqs[::-1])
    assert np.array_equal(s1, s2[::-1]) and np.array_equal(r1, r2[::-1])


@pytest.mark.parametrize("complete", [False, True], ids=["reduced", "complete"])
def test_e_backtrace(complete):
    for pool in AE.group_e(complete):
        run_pool(pool)


def test_penalties_at_and_beyond_the_header_ring():
    """mismatch and opening + extension index a ring of 64 headers: 63 is served (test_c_penalties), 64 is refused when the aligner is opened"""
    for bad in (dict(mismatch=64), dict(gap_opening=41, gap_extension=23), dict(gap_opening=0, gap_extension=64)):
        with pytest.raises(align.AlignError) as ei:
            align.Aligner(b"ACGT", workspace_bytes=AE.WORKSPACE, **bad)
        assert ei.value.code == -1
    with align.Aligner(b"ACGT", workspace_bytes=AE.WORKSPACE, mismatch=63, gap_opening=40, gap_extension=23) as al:
        score, rows = al.align([b"ACGT"])
        assert score[0] == 0 and rows[0].tobytes() == b"ACGT"
