"""The uvaiaclust kernels at their own edges: the inputs of tests/cluster_edges.py through Clusterer, clusters() and scores equal to the
CPU restatement of the reference (tests/cluster_restatement.c), rows() equal to the text.  tests/test_cluster_edges_cpu.py shows what
each input reaches."""
import pytest

import cluster_edges as E
import cluster_lib as CL
import fixtures as F
from uvaia_amd import cluster

pytestmark = pytest.mark.gpu
EALPHABET = -5


def _gpu(ref, seqs, queues, dist, trim, n_score, n_queues, ends=None, rows=False):
    """(clusters, scores[, rows() of every ordinal]); ends: where the pushes end (one push without)"""
    with cluster.Clusterer(ref, dist=dist, trim=trim, n_score=n_score, n_queues=n_queues) as c:
        a = 0
        for b in list(ends or []) + [len(seqs)]:
            c.push(seqs[a:b], queues[a:b])
            a = b
        text = c.rows(list(range(len(seqs)))) if rows else None
        c.finish()
        r = c.result()
    return (r.clusters(), r.scores, text) if rows else (r.clusters(), r.scores)


def _same(got, want, what=None):
    assert len(got[0]) == len(want[0]), what
    assert got[0] == want[0], what
    assert got[1].tolist() == want[1].tolist(), what


# ------------------------------------------------------------------------------------- A: more medoids than the LDS part of the list
def test_queue_with_more_medoids_than_lds_slots():
    ref, seqs, queues, _ = E.group_a()
    want = CL.rs_cluster(ref, seqs, queues, 0, 0, 1, 1)
    assert len(want[0]) > 14336 + 128                       # LDS_ST of uvaia_cluster.hip: if that constant moves, move cluster_edges.LDS_ST and this with it
    got = _gpu(ref, seqs, queues, 0, 0, 1, 1, ends=E.A_PUSHES)
    if got[0] != want[0]:                                   # say where, not 14 545 clusters
        wm, gm = dict(want[0]), dict(got[0])
        slot = {o: k for k, o in enumerate(sorted(wm))}
        bad = sorted(set(wm) ^ set(gm)) + [o for o in wm if o in gm and wm[o] != gm[o]]
        assert not bad, [(o, slot.get(o), wm.get(o), gm.get(o)) for o in bad[:8]]
    _same(got, want)


# ------------------------------------------------------------------------------------------------------------- B: window edges
@pytest.mark.parametrize("nchar", E.B_NCHARS)
def test_window_edges(nchar):
    cases = E.group_b_cases(nchar)
    assert cases
    for trim, p0, dist, ref, rows in cases:
        one, two = [0] * len(rows), E.alternate(len(rows))
        _same(_gpu(ref, rows, one, dist, trim, 1, 1), CL.rs_cluster(ref, rows, one, dist, trim, 1, 1), ("one queue", nchar, trim, p0, dist))
        _same(_gpu(ref, rows, two, dist, trim, 1, 2), CL.rs_cluster(ref, rows, two, dist, trim, 1, 2), ("two queues", nchar, trim, p0, dist))


# ------------------------------------------------------------------------------------------------- C: positions, counts, bytes
@pytest.mark.parametrize("trim", E.C_TRIMS)
@pytest.mark.parametrize("n_score", E.C_N_SCORES)
def test_positions_and_counts(trim, n_score):
    ref, rows, want = E.group_c(trim, n_score)
    q = [0] * len(rows)
    got = _gpu(ref, rows, q, 0, trim, n_score, 1)
    E.check_group_c(got[0], got[1], want, n_score)
    _same(got, CL.rs_cluster(ref, rows, q, 0, trim, n_score, 1))


@pytest.mark.parametrize("dist,trim,n_queues", [(0, 0, 1), (3, 5, 1), (0, 0, 3)])
def test_every_byte(dist, trim, n_queues):
    ref, rows = E.group_bytes()
    q = CL.round_robin([len(rows)], n_queues)
    got = _gpu(ref, rows, q, dist, trim, 3, n_queues, rows=True)
    assert got[2] == [r.upper() for r in rows]
    # the restatement takes the reference as the program builds it, in upper case; the device upper-cases the one it is given
    _same(got[:2], CL.rs_cluster(ref.upper(), rows, q, dist, trim, 3, n_queues))


@pytest.mark.parametrize("bad", [0x80, 0x00, 0xff])
def test_bad_byte_at_the_last_site_and_beyond(bad):
    ref = F.random_acgt(65, 77)
    last = ref[:64] + bytes([bad])                          # the one byte of the row's second 64-byte piece
    with cluster.Clusterer(ref, dist=0) as c:
        with pytest.raises(cluster.ClusterError) as ei:
            c.push([ref, last], [0, 0])
        assert ei.value.code == EALPHABET
    full = ref[:63] + bytes([bad])                          # the last byte of a full piece
    with cluster.Clusterer(ref[:64], dist=0) as c:
        with pytest.raises(cluster.ClusterError) as ei:
            c.push([full, ref[:64]], [0, 0])
        assert ei.value.code == EALPHABET
    with cluster.Clusterer(ref[:64], dist=0) as c:          # the same bytes, the bad one now beyond the 64 sites: it is not part of the row
        c.push([ref[:64], last], [0, 0])
        assert c.rows([0, 1]) == [ref[:64], ref[:64]]
        c.finish()
        assert c.result().clusters() == [(0, [1])]
    with cluster.Clusterer(ref, dist=0) as c:
        c.push([ref, sub_last(ref)], [0, 0])
        c.finish()
        assert c.result().clusters() == [(1, []), (0, [])]  # and a plain difference at site 64 counts


def sub_last(row):
    return E.sub(row, [len(row) - 1])


# ----------------------------------------------------------------------------------------------------------- D: packed pushes
def _gpu_packed(ref, pk, queues, dist, trim, n_score, n_queues):
    with cluster.Clusterer(ref, dist=dist, trim=trim, n_score=n_score, n_queues=n_queues) as c:
        c.push_packed(pk.planes, pk.n, pk.off, pk.exc, queues)
        text = c.rows(list(range(pk.n)))
        c.finish()
        r = c.result()
    return r.clusters(), r.scores, text


@pytest.mark.parametrize("nchar,n", E.D_SHAPES)
def test_packed_tile_shapes(nchar, n):
    seqs = E.group_d_rows(nchar, n)
    pk = E.Packed(seqs)
    ref = F.random_acgt(nchar, 42)
    q = CL.round_robin([n], 2)
    trim = min(3, (nchar - 1) // 2)
    want = CL.rs_cluster(ref, seqs, q, 2, trim, 1, 2)
    got = _gpu_packed(ref, pk, q, 2, trim, 1, 2)
    for i, (a, b) in enumerate(zip(got[2], pk.text)):
        assert a == b, (i, [k for k in range(nchar) if a[k] != b[k]][:8])
    _same(got[:2], want)
    _same(_gpu(ref, seqs, q, 2, trim, 1, 2), want)


@pytest.mark.parametrize("n_queues", [1, 3])
@pytest.mark.parametrize("cut", [0xFFFFFF, 5])
def test_packed_run_shapes(cut, n_queues):
    rows = E.run_rows()
    pk = E.Packed(rows, cut=cut)
    ref = rows[1].replace(b"N", b"A")
    q = CL.round_robin([len(rows)], n_queues)
    got = _gpu_packed(ref, pk, q, 0, 0, 1, n_queues)
    for i, (a, b) in enumerate(zip(got[2], rows)):
        assert a == b, (i, E.run_specs()[i // 2], [k for k in range(len(a)) if a[k] != b[k]][:8])
    _same(got[:2], CL.rs_cluster(ref, rows, q, 0, 0, 1, n_queues))


# ------------------------------------------------------ E: the medoid lists and the row arrays grow while three queues hold entries
GROW_PUSH = 150


@pytest.fixture(scope="module")
def grow():
    ref = F.random_acgt(64, 1)
    distinct = [F.random_acgt(64, 1000 + k) for k in range(800)]
    seqs = distinct + [distinct[(7 * k) % 800] for k in range(300)]
    first = {}
    for k, s in enumerate(distinct):
        first.setdefault(s, k)
    queues = [first[s] % 3 for s in seqs]
    return ref, seqs, queues, CL.rs_cluster(ref, seqs, queues, 0, 0, 2, 3)


def test_growth_input_crosses_the_first_capacities(grow):
    """what makes the growth paths matter: every queue founds more than the 256 medoid slots its lists start with, the rows pass the 1 024
    the row arrays start with, and the rows pushed after that join founders whose entries were made before the arrays grew"""
    ref, seqs, queues, want = grow
    assert len(seqs) == 1100 and len(want[0]) == 800
    founders = [m for m, _ in want[0]]
    assert sorted(founders) == list(range(800))
    assert [sum(1 for m in founders if queues[m] == q) for q in range(3)] == [267, 267, 266]
    joined = [(m, o) for m, members in want[0] for o in members]
    assert len(joined) == 300 and all(o >= 800 for _, o in joined)
    assert sum(1 for m, _ in joined if m < 768) == 290


@pytest.mark.parametrize("mode", ["default", "keep", "packed"])
def test_medoid_lists_and_rows_grow_with_contents(grow, mode):
    ref, seqs, queues, want = grow
    with cluster.Clusterer(ref, dist=0, trim=0, n_score=2, n_queues=3) as c:
        if mode == "keep":
            c.keep_medoids(4)
        for a in range(0, len(seqs), GROW_PUSH):
            b = min(a + GROW_PUSH, len(seqs))
            if mode == "packed" and a >= 600:
                pk = E.Packed(seqs[a:b])
                c.push_packed(pk.planes, pk.n, pk.off, pk.exc, queues[a:b])
            else:
                c.push(seqs[a:b], queues[a:b])
        c.finish()
        r = c.result()
        med = r.medoid.tolist()
        rows = c.rows(med)
    _same((r.clusters(), r.scores), want, mode)
    assert rows == [seqs[m] for m in med], mode
