"""derive_all_kernel with 4, 8 or 16 waves per tile (uvaia_gpu_tuning.derive_waves; 0 = the library's choice): the planes it
derives for the query set are the same byte for byte -- read back through uvaia_gpu_db_derived_export --, whether the appends wrote them
(the variant that also writes the valid-site plane) or uvaia_gpu_db_rederive did, and the search over them equals the oracle."""
import functools

import numpy as np
import pytest

import fixtures as F
import oracle_lib as O
from uvaia_amd import capi

pytestmark = pytest.mark.gpu

POOL, NBEST = 64, 5
WIDTHS = (4, 8, 16, 0)


def _n_run_queries(n, root, seed):
    """queries that differ only in their N runs: no polymorphic column at all"""
    rng = np.random.default_rng(seed)
    L, out = len(root), []
    for _ in range(n):
        s = root.copy()
        for _ in range(int(rng.integers(1, 4))):
            a = int(rng.integers(0, L))
            s[a:a + int(rng.integers(1, 60))] = ord("N")
        out.append(s.tobytes())
    return out


# name: queries, references, columns, trim, further tuning, how the queries are made
CASES = {
    "fewer_groups_than_waves": (70, 130, 333, 0, {}, "synth"),                 # W4 = 3; two tiles and a tail
    "all_boundaries_in_one_word": (70, 200, 2300, 150, {}, "few_columns"),     # W4 = 18, uneven shares, nine dense columns
    "rare_columns": (130, 200, 4097, 0, {"rare_max": 2}, "synth"),            # W4 = 33
    "no_rare_section": (200, 130, 1500, 0, {"rare_max": -1}, "synth"),
    "no_polymorphic_column": (70, 200, 2300, 0, {}, "n_runs"),
}


@functools.lru_cache(maxsize=None)
def _case(name, acgt):
    nq, nref, nchar, trim, more, how = CASES[name]
    refs, root, cols = F.synth_alignment(nref, nchar, seed=900 + nq)
    if how == "synth":
        qs, _, _ = F.synth_alignment(nq, nchar, seed=1900 + nq, root=root, poly_cols=cols, p_snp=0.004, p_amb=0.002)
    elif how == "few_columns":       # every query differs from the root on about half of nine columns inside the trimmed range
        few = np.array([160, 171, 405, 777, 901, 1302, 1303, 1777, 2100])
        qs, _, _ = F.synth_alignment(nq, nchar, seed=1900 + nq, root=root, poly_cols=few, p_snp=4.5 / nchar)
    else:
        qs = _n_run_queries(nq, root, seed=1900 + nq)
    q = O.Query(qs, ["q%d" % i for i in range(len(qs))], acgt=acgt, trim=trim)
    gold = O.search(q, refs, ["r%d" % i for i in range(nref)], pool=POOL, nbest=NBEST, ambig_r=1.0)
    return q, refs, dict(more), gold


def _check_search(eng, gold, what):
    ent = eng.search_resident(POOL)
    n, T, sc, od = eng.drain()
    assert capi.finalise_heaps(n, sc, od) == [[(tuple(s), o) for o, _, s in rows] for rows in gold.rows], what
    assert list(T) == gold.final_T, what
    assert list(np.nonzero(ent)[0]) == list(gold.saved), what


@pytest.mark.parametrize("acgt", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_every_width_derives_the_same_planes_and_the_search_equals_the_oracle(name, acgt):
    q, refs, more, gold = _case(name, acgt)
    n_tiles = (len(refs) + 63) // 64
    first = None
    for w in WIDTHS:
        with capi.Engine.from_query(q, nbest=NBEST, max_pool=128, tuning=dict(more, scan="compressed", derive_waves=w)) as eng:
            assert eng.scan_variant() == 2
            eng.db_reserve(len(refs))
            eng.db_append(refs[:70])               # (not tile aligned: the second append derives the shared tile again)
            eng.db_append(refs[70:])
            appended = eng.db_derived(n_tiles)
            _check_search(eng, gold, (w, "after the appends"))
            eng.reset()
            eng.db_rederive()
            rebuilt = eng.db_derived(n_tiles)
            _check_search(eng, gold, (w, "after a rebuild"))
        if first is None:
            first = appended
            if name == "no_polymorphic_column":
                assert first[2].size == 0
        for which, a, b, c in zip(("e", "grp", "poly", "tot"), first, appended, rebuilt):
            assert np.array_equal(a, b), (w, which, "appended")
            assert np.array_equal(a, c), (w, which, "rebuilt")
    assert first[0].any() and first[3].any()
