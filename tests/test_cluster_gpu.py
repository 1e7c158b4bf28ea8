"""uvaiaclust on the GPU: result() (medoids, member lists in order, stored score vectors) equals the CPU restatement of the reference
(tests/cluster_restatement.c) on the bundled alignment, on synthetic families and on edge cases; the command line writes the files
the restatement's clusters give."""
import lzma
import os
import subprocess

import pytest

import cluster_lib as CL
import fixtures as F
from uvaia_amd import cluster

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")


def _gpu(ref, seqs, queues, dist, trim, n_score, n_queues, batch=None):
    with cluster.Clusterer(ref, dist=dist, trim=trim, n_score=n_score, n_queues=n_queues) as c:
        batch = batch or max(len(seqs), 1)
        for a in range(0, len(seqs), batch):
            c.push(seqs[a:a + batch], queues[a:a + batch])
        c.finish()
        r = c.result()
    return r.clusters(), r.scores


def _check(ref, seqs, queues, dist, trim, n_score, n_queues, batch=None):
    want = CL.rs_cluster(ref, seqs, queues, dist, trim, n_score, n_queues)
    got = _gpu(ref, seqs, queues, dist, trim, n_score, n_queues, batch)
    assert len(got[0]) == len(want[0])
    assert got[0] == want[0]
    assert got[1].tolist() == want[1].tolist()
    return got


@pytest.fixture(scope="module")
def bundled():
    names, seqs = F.load_bundled()
    ref = CL.rs_reference(seqs[:1024])
    return names, seqs, ref


@pytest.mark.parametrize("dist,n_queues,trim,n_score", [(1, 1, 0, 1), (10, 7, 0, 1), (300, 64, 0, 1), (10, 64, 230, 3)])
def test_bundled(bundled, dist, n_queues, trim, n_score):
    _, seqs, ref = bundled
    d, t, s = CL.clamp(len(ref), dist, trim, n_score)
    # batches of 4 Q, as the command line pushes them
    _check(ref, seqs, CL.round_robin([len(seqs)], n_queues), d, t, s, n_queues, batch=4 * n_queues)


@pytest.fixture(scope="module")
def families():
    seqs = CL.families(20000, 1500, 20261016)
    return seqs, CL.rs_reference(seqs[:1024])


@pytest.mark.parametrize("dist", [3, 0])
def test_synthetic_families(families, dist):
    seqs, ref = families
    got = _check(ref, seqs, CL.round_robin([len(seqs)], 8), dist, 0, 1, 8, batch=4096)
    if dist == 3:
        assert sum(len(m) for _, m in got[0]) > len(seqs) // 4        # many joins


def test_fewer_sequences_than_queues(families):
    seqs, ref = families
    _check(ref, seqs[:5], CL.round_robin([5], 64), 3, 0, 1, 64)


def test_single_queue_and_no_snps(families):
    seqs, ref = families
    _check(ref, seqs[:3000], [0] * 3000, 3, 0, 0, 1, batch=1000)


def test_reference_given_or_built(bundled):
    _, seqs, built = bundled
    sub = seqs[:1500]
    q = CL.round_robin([len(sub)], 16)
    _check(built, sub, q, 5, 0, 1, 16)
    given = CL.rs_reference(seqs[100:101])                  # -r: the first record of the file only
    _check(given, sub, q, 5, 0, 1, 16)


def test_refuses_high_bytes():
    ref = b"ACGT" * 10
    with cluster.Clusterer(ref, dist=1) as c:
        with pytest.raises(cluster.ClusterError) as ei:
            c.push([ref, b"ACG\xc3" + ref[4:]], [0, 0])
        assert ei.value.code == -5                          # UVAIA_GPU_EALPHABET
        with pytest.raises(cluster.ClusterError):
            c.finish()


def _write(path, recs, opener=open, width=None):
    with opener(path, "wb") as fh:
        for n, s in recs:
            fh.write(b">" + n.encode() + b"\n")
            if width:
                for a in range(0, len(s), width):
                    fh.write(s[a:a + width] + b"\n")
            else:
                fh.write(s + b"\n")


def _read_fasta_text(path):
    names, seqs = F.read_fasta_bytes(lzma.open(path).read())
    return list(zip(names, seqs))


@pytest.mark.parametrize("pool,threads", [(64, 8), (3, 8)])
def test_cli_three_files(tmp_path, bundled, pool, threads):
    names, seqs, _ = bundled
    parts = [(0, 1100), (1100, 1900), (1900, 2600)]
    _write(tmp_path / "a.fa.xz", list(zip(names[0:1100], seqs[0:1100])), opener=lzma.open)
    _write(tmp_path / "b.fa", list(zip(names[1100:1900], seqs[1100:1900])), width=60)
    _write(tmp_path / "c.fa", list(zip(names[1900:2600], seqs[1900:2600])))
    files = [str(tmp_path / f) for f in ("a.fa.xz", "b.fa", "c.fa")]
    env = dict(os.environ, OMP_NUM_THREADS=str(threads))
    outs = []
    for run in range(2):
        prefix = str(tmp_path / ("out%d" % run))
        subprocess.run([UVAIACLUST, "-d", "4", "--trim", "100", "-s", "2", "-p", str(pool), "-o", prefix] + files, env=env, check=True, timeout=300,
                       capture_output=True)
        outs.append((lzma.open(prefix + ".csv.xz").read(), lzma.open(prefix + ".aln.xz").read()))
    assert outs[0] == outs[1]                               # two runs, identical files
    n_queues = max(pool, threads)
    sub_names, sub_seqs = names[:2600], seqs[:2600]
    ref = CL.rs_reference(sub_seqs[:1024])
    d, t, s = CL.clamp(len(ref), 4, 100, 2)
    clusters, _ = CL.rs_cluster(ref, sub_seqs, CL.round_robin([b - a for a, b in parts], n_queues), d, t, s, n_queues)
    assert outs[0][0].decode() == CL.csv_text(clusters, sub_names)
    got = _read_fasta_text(tmp_path / "out0.aln.xz")
    assert got == [(n, s.upper()) for n, s in CL.aln_records(clusters, sub_names, sub_seqs)]
