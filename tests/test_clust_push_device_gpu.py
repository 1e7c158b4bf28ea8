"""uvaia_clust_push_device on a GPU box: rows that are text in device memory -- any pitch, any alignment, a selection of them -- give the rows,
clusters and scores that uvaia_clust_push gives for the same text, in both residency modes and mixed with the other kinds of push; a bad
byte is reported by push ordinal, a bad pointer or index is refused before anything is pushed."""
import numpy as np
import pytest

import fixtures as F
from test_cluster_packed_gpu import Packed
from test_rows_gpu import DeviceBlock
from uvaia_amd import cluster

pytestmark = pytest.mark.gpu

EINVAL, EALPHABET, ESTATE = -1, -5, -6
N_QUEUES = 3


def _round16(x):
    return (x + 15) // 16 * 16


def _family_rows(n, nchar, seed):
    """n relatives of three roots: a few substitutions each, some lower case, N and gap runs -- many join a cluster, some found one"""
    rng = np.random.default_rng(seed)
    roots = [bytearray(F.random_acgt(nchar, seed + k)) for k in range(3)]
    rows = []
    for i in range(n):
        s = bytearray(roots[int(rng.integers(0, 3))])
        for _ in range(int(rng.integers(0, 3))):
            s[int(rng.integers(0, nchar))] = b"ACGT"[int(rng.integers(0, 4))]
        if i % 5 == 1:
            a = int(rng.integers(0, nchar))
            s[a:a + 3] = b"N-?"[:len(s[a:a + 3])]
        rows.append(bytes(s).lower() if i % 4 == 2 else bytes(s))
    return rows


def _everything(c, n, founders_only):
    """(rows, clusters, scores) of a finished context; keep medoids: the rows of the medoids"""
    c.finish()
    r = c.result()
    ords = sorted(int(m) for m in r.medoid) if founders_only else list(range(n))
    return c.rows(ords), r.clusters(), r.scores.tolist()


def _by_push(ref, rows, queues, dist, trim, keep):
    with cluster.Clusterer(ref, dist=dist, trim=trim, n_score=1, n_queues=N_QUEUES) as c:
        if keep:
            c.keep_medoids(keep)
        c.push(rows[:17], queues[:17])
        c.push(rows[17:], queues[17:])
        return _everything(c, len(rows), bool(keep))


def _by_push_device(ref, block, n, queues, dist, trim, keep):
    """the same rows in the same two pushes: the first 17 as they lie, the others through a selection"""
    with cluster.Clusterer(ref, dist=dist, trim=trim, n_score=1, n_queues=N_QUEUES) as c:
        if keep:
            c.keep_medoids(keep)
        c.push_device(block.ptr, block.pitch, queues[:17])
        c.push_device(block.ptr, block.pitch, queues[17:], row_index=list(range(17, n)))
        assert c.push_device_ms() > 0
        return _everything(c, n, bool(keep))


@pytest.mark.parametrize("nchar", [1, 15, 16, 17, 63, 64, 65, 1000])
def test_push_device_is_push(nchar):
    n = 40
    rows = _family_rows(n, nchar, seed=nchar)
    ref = F.random_acgt(nchar, nchar)
    dist, trim, _s = cluster.clamp_parameters(nchar, 2, nchar // 20, 1)
    queues = cluster.queues_round_robin([n], N_QUEUES)
    want = {keep: _by_push(ref, rows, queues, dist, trim, keep) for keep in (0, 1, 4)}
    assert want[0][0] == [r.upper() for r in rows]
    assert want[1] == want[4] and want[1][1:] == want[0][1:]
    if nchar >= 15:
        assert 1 < len(want[0][1]) < n                        # clusters were founded and joined
    for pitch in (nchar, nchar + 5, _round16(nchar)):        # rows back to back, an odd pitch, a multiple of 16
        for shift in (0, 1, 15):
            block = DeviceBlock(rows, nchar, pitch, shift)
            for keep in (0, 1, 4):
                assert _by_push_device(ref, block, n, queues, dist, trim, keep) == want[keep], (pitch, shift, keep)


def test_the_three_kinds_of_push_mix():
    nchar, n = 700, 200
    rows = [r.upper() for r in _family_rows(n, nchar, seed=9)]
    ref = F.random_acgt(nchar, 10)
    queues = cluster.queues_round_robin([n], N_QUEUES)
    with cluster.Clusterer(ref, dist=3, n_queues=N_QUEUES) as c:
        c.push(rows, queues)
        want = _everything(c, n, False)
    pk = Packed(rows[64:128])
    block = DeviceBlock(rows[128:], nchar, nchar + 3, 5)
    with cluster.Clusterer(ref, dist=3, n_queues=N_QUEUES) as c:
        c.push(rows[:64], queues[:64])
        c.push_packed(pk.planes, pk.n, pk.off, pk.exc, queues[64:128])
        c.push_device(block.ptr, block.pitch, queues[128:150])
        c.push_device(block.ptr, block.pitch, queues[150:], row_index=list(range(22, n - 128)))
        assert _everything(c, n, False) == want


def test_a_bad_byte_names_the_push_ordinal():
    nchar, n = 333, 30
    rows = _family_rows(n, nchar, seed=3)
    bad = list(rows)
    bad[21] = bad[21][:100] + b"\x80" + bad[21][101:]
    ref = F.random_acgt(nchar, 4)
    block = DeviceBlock(bad, nchar, nchar + 1, 3)
    with cluster.Clusterer(ref, dist=2, n_queues=N_QUEUES) as c:
        c.push_device(block.ptr, block.pitch, [0] * 10)
        with pytest.raises(cluster.ClusterError) as ei:
            c.push_device(block.ptr, block.pitch, [0] * 20, row_index=list(range(10, 30)))
        assert ei.value.code == EALPHABET and "sequence 21 (push ordinal)" in str(ei.value)
        with pytest.raises(cluster.ClusterError) as ei:      # the context is unusable afterwards, as after uvaia_clust_push
            c.push_device(block.ptr, block.pitch, [0] * 5)
        assert ei.value.code == ESTATE


def test_bad_pointers_and_indices_are_refused_before_anything_is_pushed():
    nchar, n = 333, 30
    rows = _family_rows(n, nchar, seed=5)
    ref = F.random_acgt(nchar, 6)
    block = DeviceBlock(rows, nchar, nchar + 1, 3)
    host = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    queues = cluster.queues_round_robin([n], N_QUEUES)
    with cluster.Clusterer(ref, dist=2, n_queues=N_QUEUES) as c:
        c.push_device(block.ptr, block.pitch, queues[:10])
        for call in (lambda: c.push_device(host.ctypes.data, nchar, queues[10:]),                                 # host memory
                     lambda: c.push_device(block.ptr, block.pitch, [0, 0], row_index=[0, 1 << 24]),               # a row beyond the allocation
                     lambda: c.push_device(block.ptr, block.pitch, [0] * (1 << 20)),                              # rows beyond the allocation
                     lambda: c.push_device(block.ptr, block.pitch, [0, 0], row_index=[3, -1]),                    # a negative row
                     lambda: c.push_device(block.ptr, nchar - 1, queues[10:]),                                    # pitch below a row
                     lambda: c.push_device(block.ptr, block.pitch, [0, N_QUEUES], row_index=[0, 1])):            # a queue out of range
            with pytest.raises(cluster.ClusterError) as ei:
                call()
            assert ei.value.code == EINVAL
            assert c.stats()["pushed"] == 10 and c.pushed == 10                  # nothing was pushed
        c.push_device(block.ptr, block.pitch, queues[10:], row_index=list(range(10, n)))      # ... and the context is usable
        got = _everything(c, n, False)
    with cluster.Clusterer(ref, dist=2, n_queues=N_QUEUES) as c:
        c.push(rows, queues)
        assert got == _everything(c, n, False)
