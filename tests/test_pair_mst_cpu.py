"""Minimum spanning tree and nearest row without a GPU: the round protocol of uvaia_gpu_db_mst, restated a step at a time in pair_mst.py,
builds Kruskal's forest edge for edge on every case; the reference README's three rows by hand; the restatements agree with each other;
the interface is declared, exported and wrapped; and what `uvaiadist --mst` / `--nearest` refuse before the engine opens."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pair_dist as D
import pair_link as K
import pair_mst as M
from uvaia_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIADIST = os.path.join(ROOT, "bin", "uvaiadist")
ENTRIES = ["uvaia_gpu_db_near_begin", "uvaia_gpu_db_near_components", "uvaia_gpu_db_near", "uvaia_gpu_db_near_fetch", "uvaia_gpu_db_mst", "uvaia_gpu_near_ms", "uvaia_gpu_near_tiles"]


def floors_of(name):
    return (0, K.SYNTH_FLOOR) if name in ("synth130", "chains260x513", "dense130") else (0, 1, 5)


@pytest.mark.parametrize("name", M.CASES)
def test_the_rounds_build_kruskals_forest(name):
    _seqs, nchar = M.case(name)
    for trim in M.trims_of(nchar):
        c = M.counts(name, trim)
        n = c.shape[0]
        for metric in ("snp", "uvaia"):
            dist, compared = M.dist_compared(c, metric)
            for floor in floors_of(name):
                want = M.kruskal_of(dist, compared >= floor)
                got, rounds = M.rounds_model(dist, compared >= floor)
                assert got == want, (trim, metric, floor)
                assert rounds <= int(np.ceil(np.log2(max(n, 2)))) + 1
                assert M.prim_of(dist, compared >= floor) == want
                assert len(want) == n - len(set(K.components(n, [(a, b) for a, b, _d in want]).tolist()))
                # cutting the tree at D gives the clusters at D
                for max_dist in (0, 1, 2):
                    assert np.array_equal(M.components_at(n, want, max_dist), K.restate(c, metric, max_dist, floor)[0])


def test_all_ties_give_the_star_on_the_first_row():
    c = M.counts("dense130")
    for metric in ("snp", "uvaia"):
        want = [(0, i, 0) for i in range(1, 130)]
        assert M.kruskal(c, metric) == want
        dist, compared = M.dist_compared(c, metric)
        got, rounds = M.rounds_model(dist, compared >= 0)
        assert got == want and rounds == 1
        best = M.nearest(c, metric)
        assert int(best[0]) == 1 and not best[1:].any()            # (0 << 32 | 1, and 0 << 32 | 0 for everyone else)


def test_two_components_choose_the_same_edge():
    """rows 0 and 1 are each other's nearest: the edge comes from both sides and goes in once"""
    dist = np.array([[0, 1, 5, 6], [1, 0, 7, 8], [5, 7, 0, 2], [6, 8, 2, 0]], dtype=np.int64)
    edge = np.ones((4, 4), dtype=bool)
    best = M.nearest_of(dist, edge)
    assert [int(b) & 0xFFFFFFFF for b in best] == [1, 0, 3, 2]
    got, rounds = M.rounds_model(dist, edge)
    assert got == M.kruskal_of(dist, edge) == [(0, 1, 1), (2, 3, 2), (0, 2, 5)] and rounds == 2


def test_the_readme_toy_by_hand():
    """AACGTTA-- / AACG-TAM- / MNCGTTMC-: every pair agrees wherever both rows are ACGT (6, 4 and 3 sites) and wherever both are valid, so
    every distance is 0 and the order alone decides: the star on the first row; a floor of 5 ACGT sites leaves the one edge {0, 1}"""
    c = M.counts("toy")
    assert D.snp(c)[np.triu_indices(3, 1)].tolist() == [0, 0, 0] and c[..., 4][np.triu_indices(3, 1)].tolist() == [6, 4, 3]
    assert D.uvaia(c)[np.triu_indices(3, 1)].tolist() == [0, 0, 0]
    for metric in ("snp", "uvaia"):
        assert M.kruskal(c, metric) == [(0, 1, 0), (0, 2, 0)]
        assert [int(b) for b in M.nearest(c, metric)] == [1, 0, 0]
    assert M.kruskal(c, "snp", 4) == [(0, 1, 0), (0, 2, 0)]
    assert M.kruskal(c, "snp", 5) == [(0, 1, 0)]
    assert [int(b) for b in M.nearest(c, "snp", 5)] == [1, 0, M.NONE]
    assert M.mst_text(M.TOY_NAMES, M.kruskal(c, "snp")) == b"seq1\tseq2\t0\nseq1\tseq3\t0\n"
    assert M.nearest_text(M.TOY_NAMES, M.nearest(c, "snp", 5), sep=",") == b"seq1,seq2,0\nseq2,seq1,0\nseq3,,-1\n"


def test_the_hub_under_snp_and_the_floor_against_it():
    c = M.counts("special129")
    assert M.kruskal(c, "snp") == [(0, i, 0) for i in range(1, 6)]   # the all-N row is at distance 0 from everything
    floor = M.kruskal(c, "snp", 1)
    assert all(a >= 3 for a, _b, _d in floor) and len(floor) == 2      # rows 0, 1, 2 have no ACGT site: trees of their own
    assert [int(b) for b in M.nearest(c, "snp", 1)[:3]] == [M.NONE] * 3


def test_nearest_with_components():
    c = M.counts("synth130")
    n = 130
    dist, _compared = M.dist_compared(c, "snp")
    for comp in (np.arange(n), np.zeros(n), np.arange(n) // 64, np.arange(n) % 2, np.arange(n) // 32):
        best = M.nearest(c, "snp", 0, comp)
        for x in range(n):
            other = [(int(dist[x, y]), y) for y in range(n) if comp[y] != comp[x]]
            assert int(best[x]) == (min(other)[0] << 32 | min(other)[1] if other else M.NONE)


def test_the_matrix_product_restatement_of_both_distances():
    seqs, _nchar = K.case("special129")
    seqs = seqs + K.case("awkward9x129")[0]
    rows = np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), -1)
    for trim in (0, 33):
        c = D.oracle_counts_of(seqs, trim)
        for metric in ("snp", "uvaia"):
            dist, compared = M.dist_of_bytes(rows, trim, metric, block=4)
            want_d, want_c = M.dist_compared(c, metric)
            assert np.array_equal(dist, want_d) and np.array_equal(compared, want_c), (trim, metric)


def test_the_launch_cut_rows_have_ties_and_duplicates():
    rows = M.launch_cut_rows()
    assert rows.shape == (2100, 129) and set(np.unique(rows).tolist()) == set(b"ACGT")
    dist, compared = M.dist_of_bytes(rows[:300], 0, "snp")
    assert (compared == 129).all() and (dist[np.triu_indices(300, 1)] == 0).sum() > 0
    edge = np.ones_like(dist, dtype=bool)
    assert M.prim_of(dist, edge) == M.kruskal_of(dist, edge) == M.rounds_model(dist, edge)[0]


def test_the_tile_counters_of_the_skip_case():
    """one outsider: exactly the tile pairs that hold it, in rows or columns, are walked"""
    for outsider in M.SKIP_OUTSIDERS:
        walked, skipped = M.tile_stats(M.skip_comp(outsider), "snp")
        assert walked + skipped == 7 * 4                              # seven row tiles of 32 x four column tiles, one launch
        assert walked == 4 + 7 - 1, outsider                          # its row tile against every column tile, its column tile under every row tile
    assert M.tile_stats(np.zeros(200), "snp") == (0, 28) and M.tile_stats(np.arange(200), "uvaia") == (13 * 4, 0)
    assert M.tile_stats(np.arange(200) // 64, "snp") == (28 - 7, 7)  # the column tiles on the diagonal: two row tiles over each, one over the last
    assert M.tile_stats(np.zeros(200), "snp", rows=(130, 70), cols=(0, 130)) == (0, 0)      # wholly below the diagonal: nothing is launched


# ---- the interface
def test_the_header_declares_the_entries_and_the_library_exports_them():
    header = open(os.path.join(ROOT, "include", "uvaia_gpu.h")).read()
    for name in ENTRIES:
        assert re.search(r"^(int|void)\s+%s \(uvaia_gpu_ctx \*ctx" % name, header, re.M), name
    assert re.search(r"typedef struct \{ uint32_t a, b; int32_t dist; \} uvaia_gpu_edge;", header)
    assert "#define UVAIA_GPU_NEAR_NONE UINT64_MAX" in header
    lib = ctypes.CDLL(os.path.join(ROOT, "uvaia_amd", "lib", "libuvaia_gpu.so"))
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_capi_has_the_wrappers():
    assert all(name in capi.SYMBOLS for name in ENTRIES)
    for method in ("db_near_begin", "db_near_components", "db_near", "db_near_fetch", "db_mst", "near_ms", "near_tiles"):
        assert callable(getattr(capi.Engine, method))
    assert capi.EDGE_DTYPE.itemsize == 12 and capi.NEAR_NONE == M.NONE


# ---- uvaiadist: what is refused before the engine opens, each by its own message
@pytest.mark.parametrize("form", ["--mst", "--nearest"])
@pytest.mark.parametrize("args, message", [
    (("-d", "1"), "%s does not go with -d"),
    (("-d", "1", "--clusters"), "%s does not go with -d"),
    (("--clusters",), "%s does not go with --clusters"),
    (("--long",), "%s does not go with --long"),
    (("--counts",), "%s does not go with --counts"),
    (("--dense",), "%s does not go with --dense"),
    (("--min-size", "2"), "%s does not go with --min-size"),
    (("--min-compared", "-1"), "--min-compared takes a number of 0 or more"),
])
def test_refusals_need_no_gpu(form, args, message):
    r = subprocess.run([UVAIADIST, form, *args, "--stdout", "x.fa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0
    assert (message % form if "%s" in message else message).encode() in r.stderr, r.stderr
    assert not r.stdout


def test_the_two_forms_exclude_each_other_and_the_old_message_stays():
    r = subprocess.run([UVAIADIST, "--mst", "--nearest", "--stdout", "x.fa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0 and b"--mst and --nearest are two forms of the output: give one" in r.stderr and not r.stdout
    r = subprocess.run([UVAIADIST, "--min-compared", "5", "--stdout", "x.fa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0 and r.stderr == b"--min-compared needs --clusters: it decides which pairs link two sequences\n" and not r.stdout
