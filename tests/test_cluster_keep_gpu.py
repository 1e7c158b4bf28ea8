"""The "keep medoids" mode of the clusterer (uvaia_clust_keep_medoids: only the sequences that found a cluster stay in device memory, in
slabs) on the GPU.  The reference of every comparison is the CPU restatement (tests/cluster_restatement.c through cluster_lib), the default
mode on the same pushes is a second witness: clusters, member lists, scores and the medoid rows.  Then the command line."""
import lzma
import os
import subprocess

import numpy as np
import pytest

import cluster_edges as E
import cluster_lib as CL
import fixtures as F
import oracle_lib as O
import rows_lib as R
from uvaia_amd import capi, cluster

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")
EINVAL, ESTATE = -1, -6


def _cuts(n, size):
    return list(range(size, n, size)) if size else []


def _gpu(ref, seqs, queues, dist, trim, n_score, n_queues, ends=None, slab=None, packed_from=None):
    """(clusters, scores, {founder ordinal: row}, memory()); ends: where the pushes end; slab: keep medoids with this slab_rows (None: the
    default mode, where the rows of the final medoids are fetched); packed_from: the pushes that start at or after this ordinal are packed"""
    with cluster.Clusterer(ref, dist=dist, trim=trim, n_score=n_score, n_queues=n_queues) as c:
        if slab is not None:
            c.keep_medoids(slab)
        a = 0
        for b in list(ends or []) + [len(seqs)]:
            if packed_from is not None and a >= packed_from:
                pk = E.Packed(seqs[a:b])
                c.push_packed(pk.planes, pk.n, pk.off, pk.exc, queues[a:b])
            else:
                c.push(seqs[a:b], queues[a:b])
            a = b
        c.finish()
        r = c.result()
        med = r.medoid.tolist()
        rows = dict(zip(med, c.rows(med)))
        mem = c.memory()
    return r.clusters(), r.scores, rows, mem


def _check(got, want, seqs, what=None):
    assert got[0] == want[0], what
    assert got[1].tolist() == want[1].tolist(), what
    assert got[2] == {m: seqs[m].upper() for m, _ in want[0]}, what


# ------------------------------------------------------------------- 1: founders of the same push and of earlier pushes
FAM_N = 150


@pytest.fixture(scope="module")
def fam():
    seqs = CL.families(FAM_N, 12, 20261018)
    return seqs, CL.rs_reference(seqs)


@pytest.mark.parametrize("n_queues", [1, 3, FAM_N + 7])
@pytest.mark.parametrize("dist", [0, 1, 3])
def test_families_in_pushes_of_every_size(fam, dist, n_queues):
    seqs, ref = fam
    q = CL.round_robin([len(seqs)], n_queues)
    want = CL.rs_cluster(ref, seqs, q, dist, 0, 1, n_queues)
    assert 1 < len(want[0]) < len(seqs) or dist == 0                # rows that found and rows that join
    _check(_gpu(ref, seqs, q, dist, 0, 1, n_queues, ends=_cuts(len(seqs), 64)), want, seqs, "default mode")
    for size in (1, 5, 64, 0):
        _check(_gpu(ref, seqs, q, dist, 0, 1, n_queues, ends=_cuts(len(seqs), size), slab=4), want, seqs, ("pushes of", size))
    _check(_gpu(ref, seqs, q, dist, 0, 1, n_queues, ends=_cuts(len(seqs), 64), slab=0), want, seqs, "default slab size")


@pytest.mark.parametrize("n_queues", [1, 2])
def test_a_push_where_every_row_joins_and_one_where_every_row_founds(n_queues):
    ref = F.random_acgt(61, 1)
    distinct = [F.random_acgt(61, 100 + k) for k in range(23)]
    seqs = distinct[:7] + [distinct[k % 7] for k in range(10)] + distinct[7:] + distinct[::-1]
    ends = [7, 17, 17 + 16]                                          # 7 founders; 10 rows that all join; 16 founders; 23 rows that all join
    q = [distinct.index(s) % n_queues for s in seqs]                 # a copy goes to the queue of its original: it joins in phase 2
    want = CL.rs_cluster(ref, seqs, q, 0, 0, 1, n_queues)
    assert len(want[0]) == 23 and sorted(m for m, _ in want[0]) == list(range(7)) + list(range(17, 33))
    for slab in (1, 2, 4, 8):
        _check(_gpu(ref, seqs, q, 0, 0, 1, n_queues, ends=ends, slab=slab), want, seqs, slab)
    _check(_gpu(ref, seqs, q, 0, 0, 1, n_queues, ends=ends), want, seqs)


# ------------------------------------------------------------------------------------------------------------ 2: slab edges
@pytest.mark.parametrize("founders", [9, 12])
@pytest.mark.parametrize("slab", [1, 2, 4])
def test_founders_of_one_push_straddle_slabs(slab, founders):
    nchar = 130
    ref = F.random_acgt(nchar, 2)
    distinct = [F.random_acgt(nchar, 200 + k) for k in range(founders)]
    seqs = []
    for k, s in enumerate(distinct):                                 # every founder followed by a copy of an earlier one
        seqs += [s, distinct[k // 2]]
    q = [0] * len(seqs)
    want = CL.rs_cluster(ref, seqs, q, 0, 0, 1, 1)
    assert len(want[0]) == founders
    for ends in (_cuts(len(seqs), 10), [], _cuts(len(seqs), 3)):     # pushes of 10 rows hold 5 founders: slots 0-4, 5-9, ... cross every slab size
        with cluster.Clusterer(ref, dist=0) as c:
            c.keep_medoids(slab)
            a = 0
            for b in ends + [len(seqs)]:
                c.push(seqs[a:b], q[a:b])
                a = b
                have = [o for o in range(0, b, 2)]                   # the founders so far: their rows before finish
                assert c.rows(have) == [seqs[o] for o in have]
            mem = c.memory()
            assert mem["row_bytes"] == (-(-founders // slab) * slab + max(b - a for a, b in zip([0] + ends, ends + [len(seqs)]))) * 192
            c.finish()
            r = c.result()
            assert r.clusters() == want[0] and r.scores.tolist() == want[1].tolist()
            order = list(range(len(seqs) - 2, -1, -2)) + [0, 0]
            assert c.rows(order) == [seqs[o] for o in order]


# ------------------------------------------------------------------------------------------- 3: the shapes of cluster_edges
def test_queue_with_more_medoids_than_lds_slots():
    ref, seqs, queues, _ = E.group_a()
    want = CL.rs_cluster(ref, seqs, queues, 0, 0, 1, 1)
    assert len(want[0]) > E.LDS_ST + 128
    with cluster.Clusterer(ref, dist=0, trim=0, n_score=1, n_queues=1) as c:
        c.keep_medoids(4)
        a = 0
        for b in list(E.A_PUSHES) + [len(seqs)]:
            c.push(seqs[a:b], queues[a:b])
            a = b
        c.finish()
        r = c.result()
        probe = [m for m, _ in want[0]][::997]
        assert c.rows(probe) == [seqs[m] for m in probe]
    assert r.clusters() == want[0]
    assert r.scores.tolist() == want[1].tolist()


@pytest.mark.parametrize("nchar", [63, 64, 65, 1000])
def test_window_edges(nchar):
    cases = E.group_b_cases(nchar)
    assert any(trim > 0 for trim, _, _, _, _ in cases)
    for trim, p0, dist, ref, rows in cases:
        one, two = [0] * len(rows), E.alternate(len(rows))
        for q, nq in ((one, 1), (two, 2)):
            want = CL.rs_cluster(ref, rows, q, dist, trim, 1, nq)
            _check(_gpu(ref, rows, q, dist, trim, 1, nq, slab=4), want, rows, (nchar, trim, p0, dist, nq))
            _check(_gpu(ref, rows, q, dist, trim, 1, nq, ends=_cuts(len(rows), 3), slab=4), want, rows, (nchar, trim, p0, dist, nq, "pushes of 3"))


@pytest.mark.parametrize("trim", E.C_TRIMS)
@pytest.mark.parametrize("n_score", E.C_N_SCORES)
def test_positions_and_counts(trim, n_score):
    ref, rows, want = E.group_c(trim, n_score)
    q = [0] * len(rows)
    got = _gpu(ref, rows, q, 0, trim, n_score, 1, ends=_cuts(len(rows), 7), slab=4)
    E.check_group_c(got[0], got[1], want, n_score)
    _check(got, CL.rs_cluster(ref, rows, q, 0, trim, n_score, 1), rows)


# ------------------------------------------------------------------------------------------------------ 4: packed pushes
@pytest.mark.parametrize("nchar,n", [(129, 65), (129, 130), (777, 130)])
def test_packed_and_text_pushes(nchar, n):
    seqs = E.group_d_rows(nchar, n)
    last = bytearray(seqs[3])
    last[nchar - 5:] = b"-" * 5                                      # a run that ends at the row's last site
    seqs[3] = bytes(last)
    assert len(cluster.exception_runs([s.upper() for s in seqs])[1]) > n // 4
    seqs = seqs + seqs[:10]                                          # and rows that join
    text = [s.upper() for s in seqs]
    ref = F.random_acgt(nchar, 42)
    q = CL.round_robin([len(seqs)], 2)
    trim = 3
    want = CL.rs_cluster(ref, seqs, q, 2, trim, 1, 2)
    assert len(want[0]) < len(seqs)
    _check(_gpu(ref, seqs, q, 2, trim, 1, 2, ends=[n], slab=4, packed_from=0), want, text, "packed: n rows, then 10")
    _check(_gpu(ref, seqs, q, 2, trim, 1, 2, ends=[40], slab=4, packed_from=40), want, text, "text, then packed")
    _check(_gpu(ref, seqs, q, 2, trim, 1, 2, ends=[n], slab=4, packed_from=n), want, text, "text, then the rest packed")
    got = _gpu(ref, seqs, q, 2, trim, 1, 2, ends=[n], packed_from=0)
    _check(got, want, text, "default mode")


# ------------------------------------------------------------------------------------------------ 5: rows and the refusals
def test_rows_of_founders_and_the_refusals():
    nchar = 200
    ref = F.random_acgt(nchar, 5)
    a, b = F.random_acgt(nchar, 6), F.random_acgt(nchar, 7)
    seqs = [a, a.lower(), a, b, b, a]                                # queues 0 1 0 1 0 1: ordinal 1 founds in queue 1 and is absorbed by 0's cluster
    q = [0, 1, 0, 1, 0, 1]
    want = CL.rs_cluster(ref, seqs, q, 0, 0, 1, 2)
    assert want[0] == [(0, [2, 1, 5]), (4, [3])]                     # the merge absorbs the clusters ordinals 1 and 3 founded in queue 1
    founders, joined = [0, 1, 3, 4], [2, 5]
    with cluster.Clusterer(ref, dist=0, n_queues=2) as c:
        c.push(seqs, q)
        all_rows = c.rows(list(range(6)))
        p, pitch = c.device_rows()
        assert p and pitch == 256
        c.finish()
        with pytest.raises(cluster.ClusterError) as ei:
            c.keep_medoids(4)                                        # after a push
        assert ei.value.code == ESTATE
        keep_all = c.result()
    with cluster.Clusterer(ref, dist=0, n_queues=2) as c:
        for bad in (3, 6, 12, -1, -4):
            with pytest.raises(cluster.ClusterError) as ei:
                c.keep_medoids(bad)
            assert ei.value.code == EINVAL
        c.keep_medoids(2)
        c.push(seqs[:4], q[:4])
        with pytest.raises(cluster.ClusterError) as ei:
            c.keep_medoids(2)
        assert ei.value.code == ESTATE
        c.push(seqs[4:], q[4:])
        for when in ("before finish", "after finish"):
            assert c.rows(founders) == [all_rows[o] for o in founders], when
            for o in joined:
                with pytest.raises(cluster.ClusterError) as ei:
                    c.rows([0, o])
                assert ei.value.code == EINVAL, when
                assert c.rows([3, 0]) == [all_rows[3], all_rows[0]], when                  # the context stays usable
            with pytest.raises(cluster.ClusterError) as ei:
                c.rows([6])
            assert ei.value.code == EINVAL
            with pytest.raises(cluster.ClusterError) as ei:
                c.device_rows()
            assert ei.value.code == ESTATE and "uvaia_clust_gather_device" in str(ei.value)
            if when == "before finish":
                c.finish()
        r = c.result()
        assert r.clusters() == want[0] == keep_all.clusters()
        assert 1 not in r.medoid.tolist()                            # ordinal 1 founded a cluster that the merge absorbed: its row is still there
        assert c.rows([1]) == [a]


# ------------------------------------------------------------------------------------------------------------- 6: memory
def test_memory_follows_the_founders_not_the_rows():
    seqs = CL.families(512, 8, 20261019)
    ref = CL.rs_reference(seqs)
    pitch = (len(ref) + 63) // 64 * 64
    q = [0] * len(seqs)
    want = CL.rs_cluster(ref, seqs, q, 3, 0, 1, 1)
    M = len(want[0])                                                 # one queue: no merge, every cluster is one founder of phase 2
    bound = ((M + 7) // 8 + 1) * 8 * pitch + 64 * pitch
    assert bound < 512 * pitch, M                                    # the two conditions below differ on this input
    keep = _gpu(ref, seqs, q, 3, 0, 1, 1, ends=_cuts(512, 64), slab=8)
    _check(keep, want, seqs)
    print("founders %d, peak row bytes %d, bound %d, 512 rows %d" % (M, keep[3]["peak_row_bytes"], bound, 512 * pitch))
    assert 0 < keep[3]["row_bytes"] <= keep[3]["peak_row_bytes"] <= bound
    assert keep[3]["free_bytes"] > 0
    every = _gpu(ref, seqs, q, 3, 0, 1, 1, ends=_cuts(512, 64))
    _check(every, want, seqs)
    assert every[3]["peak_row_bytes"] >= 512 * pitch and every[3]["row_bytes"] >= 512 * pitch


# ----------------------------------------------------------------------------------------- 7: medoid rows for the packer
def _query(nchar):
    root = F.random_acgt(nchar, 3)
    return O.Query([root, E.sub(root, [5, 77])], ["q0", "q1"])


def test_gathered_rows_feed_the_census_and_the_resident_database():
    nchar, n = 1237, 150
    rows = R.random_rows(n, nchar, seed=11, special=True)
    seqs = rows + rows[:40]
    ref = F.random_acgt(nchar, 12)
    q = CL.round_robin([len(seqs)], 3)
    out = {}
    for mode in ("every row", "medoids"):
        with cluster.Clusterer(ref, dist=1, n_queues=3) as c, capi.Engine.from_query(_query(nchar), nbest=4, max_pool=64) as eng:
            if mode == "medoids":
                c.keep_medoids(4)
            for a in range(0, len(seqs), 64):
                c.push(seqs[a:a + 64], q[a:a + 64])
            c.finish()
            med = c.result().medoid.tolist()
            eng.db_reserve(len(med) + 64)
            if mode == "every row":
                p, pitch = c.device_rows()
                non_n, n_exc = eng.rows_census(p, pitch=pitch, n=len(seqs))
                non_n, n_exc = non_n[med], n_exc[med]
                recs = eng.rows_exceptions(p, n_exc, row_index=med, pitch=pitch, n=len(seqs))
                eng.db_append_device(p, row_index=med, pitch=pitch, n=len(seqs))
            else:
                p, pitch = c.gather_device(med)
                non_n, n_exc = eng.rows_census(p, pitch=pitch, n=len(med))
                recs = eng.rows_exceptions(p, n_exc, pitch=pitch, n=len(med))
                eng.db_append_device(p, pitch=pitch, n=len(med))
                with pytest.raises(cluster.ClusterError) as ei:
                    c.gather_device([med[0], 150])                      # ordinal 150 repeats row 0 in row 0's queue (150 = 0 mod 3): it joined
                assert ei.value.code == EINVAL
            out[mode] = (med, non_n.tolist(), n_exc.tolist(), recs[0].tolist(), recs[1].tolist()) + tuple(x.tolist() for x in eng.db_export())
    assert len(out["medoids"][0]) > 64 and sum(out["medoids"][2]) > 0
    assert out["medoids"] == out["every row"]
    assert out["medoids"][1] == [R.count_non_n(seqs[m]) for m in out["medoids"][0]]
    with cluster.Clusterer(ref, dist=1, n_queues=3) as c, capi.Engine.from_query(_query(nchar), nbest=4, max_pool=64) as eng:
        c.push(seqs, q)
        some = [5, 0, 189, 5]                                        # the default mode gathers any pushed row
        p, pitch = c.gather_device(some)
        assert eng.rows_census(p, pitch=pitch, n=len(some))[0].tolist() == [R.count_non_n(seqs[m]) for m in some]


# ---------------------------------------------------------------------------------------------------------- 8: command line
def _run(cmd, env=None):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900, env=env)
    assert r.returncode == 0, (cmd, r.stderr[-3000:])
    return r.stderr.decode(errors="replace")


def _xz(path):
    return lzma.open(path, "rb").read()


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("clust_keep")
    aln = os.path.join(ROOT, "tests", "golden", "03.unique_acgt.aln.xz")
    _run([UVAIAPACK, "-A", "1", "-o", str(d / "in.uvdb"), aln])
    return d, aln, dict(os.environ, OMP_NUM_THREADS="8")


@pytest.mark.parametrize("dist", [1, 10])
@pytest.mark.parametrize("source", ["text", "packed"])
def test_cli_keep_medoids_writes_the_same_files(work, source, dist):
    d, aln, env = work
    inp = [aln] if source == "text" else ["--packed", str(d / "in.uvdb")]
    base = ["-d", str(dist), "--trim", "100", "-p", "64"]
    tag = "%s%d" % (source, dist)
    e0 = _run([UVAIACLUST] + base + ["--packed-out", str(d / (tag + "_all.uvdb")), "-o", str(d / (tag + "_all"))] + inp, env)
    e1 = _run([UVAIACLUST] + base + ["--keep-medoids", "--packed-out", str(d / (tag + "_keep.uvdb")), "-o", str(d / (tag + "_keep"))] + inp, env)
    assert "every row kept" in e0 and "medoid rows in slabs" in e1 and "Keeping medoid rows only" not in e0
    assert _xz(d / (tag + "_keep.csv.xz")) == _xz(d / (tag + "_all.csv.xz"))
    assert _xz(d / (tag + "_keep.aln.xz")) == _xz(d / (tag + "_all.aln.xz"))
    assert len(_xz(d / (tag + "_keep.csv.xz")).splitlines()) > 64
    assert (d / (tag + "_keep.uvdb")).read_bytes() == (d / (tag + "_all.uvdb")).read_bytes()
