"""uvaiaclust from a packed database on the GPU: push_packed gives the clusters of the CPU restatement (tests/cluster_restatement.c) run on
the upper-case text, however the database is cut into pushes and mixed with text pushes; the exception runs decide; rows() gives the exact
text back; `uvaiaclust --packed` writes the files the text command writes, and --packed-out the file `uvaiapack` makes of <prefix>.aln.xz."""
import lzma
import os
import subprocess

import numpy as np
import pytest

import cluster_lib as CL
import fixtures as F
import packed_lib as P
import rows_lib as R
from uvaia_amd import cluster

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIA = os.path.join(ROOT, "bin", "uvaia")
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")
EINVAL = -1


class Packed:
    """sequences as a packed database holds them: whole tiles and exception runs of the upper-case text"""

    def __init__(self, seqs):
        self.text = [s.upper() for s in seqs]
        self.n, self.nchar = len(seqs), len(seqs[0])
        self.tile = P.tile_bytes(self.nchar)
        self.planes = np.concatenate([P.pack_tiles(self.text[a:a + 1280], self.nchar)[0] for a in range(0, self.n, 1280)])
        self.off, self.exc = cluster.exception_runs(self.text)

    def push(self, c, a, b, queues):
        """sequences a .. b (a on a tile boundary)"""
        assert a % 64 == 0
        c.push_packed(self.planes[a // 64:(b + 63) // 64], b - a, self.off[a:b + 1], self.exc, queues[a:b])


def _gpu_packed(ref, pk, queues, dist, trim, n_score, n_queues, chunk=None, text_until=0):
    with cluster.Clusterer(ref, dist=dist, trim=trim, n_score=n_score, n_queues=n_queues) as c:
        if text_until:
            c.push(pk.text[:text_until], queues[:text_until])
        chunk = chunk or max(pk.n, 1)
        for a in range(text_until, pk.n, chunk):
            pk.push(c, a, min(pk.n, a + chunk), queues)
        c.finish()
        r = c.result()
        ms = c.unpack_ms()
    assert ms["decode_ms"] > 0
    return r.clusters(), r.scores


def _same(got, want):
    assert len(got[0]) == len(want[0])
    assert got[0] == want[0]
    assert got[1].tolist() == want[1].tolist()


@pytest.fixture(scope="module")
def bundled():
    names, seqs = F.load_bundled()
    return names, seqs, CL.rs_reference(seqs[:1024]), Packed(seqs)


@pytest.mark.parametrize("dist,n_queues,trim,n_score", [(1, 1, 0, 1), (10, 7, 0, 1), (300, 64, 0, 1), (10, 64, 230, 3)])
def test_api_parity_on_the_bundled_alignment(bundled, dist, n_queues, trim, n_score):
    _, seqs, ref, pk = bundled
    assert pk.n % 64 != 0                                    # the last tile is ragged
    d, t, s = CL.clamp(len(ref), dist, trim, n_score)
    q = CL.round_robin([pk.n], n_queues)
    want = CL.rs_cluster(ref, pk.text, q, d, t, s, n_queues)
    _same(_gpu_packed(ref, pk, q, d, t, s, n_queues), want)                  # one push
    _same(_gpu_packed(ref, pk, q, d, t, s, n_queues, chunk=4096), want)
    _same(_gpu_packed(ref, pk, q, d, t, s, n_queues, chunk=64), want)        # tile by tile, the last one ragged
    half = pk.n // 2 // 64 * 64
    _same(_gpu_packed(ref, pk, q, d, t, s, n_queues, chunk=4096, text_until=half), want)      # half as text, half packed


# ------------------------------------------------------------------------------------------------------------ exceptions decide
NCHAR, DIST = 700, 3


def _put(s, a, b, ch):
    s = bytearray(s)
    s[a:b] = ch * (b - a)
    return bytes(s)


def _snp(s, sites):
    s = bytearray(s)
    for k in sites:
        s[k] = ord("A") if s[k] != ord("A") else ord("C")
    return bytes(s)


def exception_rows():
    base = [F.random_acgt(NCHAR, 100 + k) for k in range(12)]
    rows = []
    # (a) the same stretch as '-' in one row and as 'N' in the other: 10 differences in the window, more than d
    rows += [_put(base[0], 200, 210, b"-"), _put(base[0], 200, 210, b"N")]
    # (b) the same '-' and '?' runs in both, two other sites differ: within d
    b1 = _put(_put(base[1], 300, 340, b"-"), 400, 405, b"?")
    rows += [b1, _snp(b1, [50, 600])]
    # (c) runs from site 0, up to the last site, across word (32 sites) and word-group (128 sites) boundaries, over several word groups,
    #     three sites long: each with a twin that has 'N' there
    for k, (a, b, ch) in enumerate([(0, 9, b"-"), (NCHAR - 7, NCHAR, b"?"), (120, 140, b"X"), (250, 262, b"O"), (380, 650, b"."), (30, 33, b"-")]):
        rows += [_put(base[2 + k], a, b, ch), _put(base[2 + k], a, b, b"N")]
    # inside the margins a trim of 20 cuts off, and nowhere else: the twin joins whatever is read there
    rows += [_put(_put(base[8], 3, 15, b"-"), NCHAR - 15, NCHAR - 4, b"?"), _put(_put(base[8], 3, 15, b"N"), NCHAR - 15, NCHAR - 4, b"N")]
    # whole rows
    rows += [b"-" * NCHAR, b"N" * NCHAR, b"?" * NCHAR]
    return rows


@pytest.mark.parametrize("trim,n_queues", [(20, 1), (0, 3), (0, 1)])
def test_exception_runs_decide(trim, n_queues):
    rows = exception_rows()
    ref = F.random_acgt(NCHAR, 99)
    q = CL.round_robin([len(rows)], n_queues)
    want = CL.rs_cluster(ref, rows, q, DIST, trim, 1, n_queues)
    pk = Packed(rows)
    # what a decode that drops the runs would cluster: the planes alone read N at every one of these sites
    bare = [P.decode_reference(pk.planes, i, NCHAR) for i in range(len(rows))]
    assert bare != rows
    blind = CL.rs_cluster(ref, bare, q, DIST, trim, 1, n_queues)
    assert blind[0] != want[0] and len(blind[0]) < len(want[0])
    members = {m: mem for m, mem in want[0]}
    if n_queues == 1:
        assert members[0] == [] and members[1] == []         # (a) stay apart
        assert members[2] == [3]                             # (b) merge
        assert members[16] == ([17] if trim else [])         # margins: only the trim hides the difference
        assert members[18] == [] and members[19] == [] and members[20] == []
    got = _gpu_packed(ref, pk, q, DIST, trim, 1, n_queues)
    _same(got, want)
    with cluster.Clusterer(ref, dist=DIST, trim=trim, n_score=1, n_queues=n_queues) as c:
        pk.push(c, 0, pk.n, q)
        assert c.rows(list(range(pk.n))) == rows
        assert c.unpack_ms()["overlay_ms"] > 0


def test_not_vacuous_on_synthetic_families():
    seqs = CL.families(20000, 1500, 20261017)
    rng = np.random.default_rng(5)
    for i in range(0, len(seqs), 10):                        # exception runs in a tenth of the rows
        a = bytearray(seqs[i])
        p, k = int(rng.integers(0, len(a) - 200)), int(rng.integers(1, 200))
        a[p:p + k] = bytes([b"-?XO."[i // 10 % 5]]) * k
        seqs[i] = bytes(a)
    ref = CL.rs_reference(seqs[:1024])
    q = CL.round_robin([len(seqs)], 8)
    want = CL.rs_cluster(ref, seqs, q, 3, 0, 1, 8)
    got = _gpu_packed(ref, Packed(seqs), q, 3, 0, 1, 8, chunk=4096)
    _same(got, want)
    assert sum(len(m) for _, m in got[0]) > len(seqs) // 4   # many joins


def test_rows_returns_the_exact_text():
    nchar = 1003                                             # not a multiple of 16: the last piece of a row is cut
    seqs = P.awkward_references(150, nchar, seed=41)         # three tiles, the last one ragged; lower case, every exception character
    pk = Packed(seqs)
    ref = F.random_acgt(nchar, 42)
    rng = np.random.default_rng(43)
    order = rng.permutation(pk.n).tolist() + rng.integers(0, pk.n, 60).tolist() + [0, 0, pk.n - 1, pk.n - 1]
    with cluster.Clusterer(ref, dist=2, n_queues=4) as c:
        q = CL.round_robin([pk.n], 4)
        pk.push(c, 0, 128, q)
        assert c.rows(order[:0]) == []
        assert c.rows([127, 0, 127]) == [pk.text[127], pk.text[0], pk.text[127]]
        c.push(seqs[128:], q[128:])                          # the rest as text, lower case and all: rows() gives it back in upper case
        before = c.rows(order)
        c.finish()
        after = c.rows(order)
        with pytest.raises(cluster.ClusterError) as ei:
            c.rows([pk.n])
        assert ei.value.code == EINVAL
    assert before == [pk.text[o] for o in order]
    assert after == before


@pytest.mark.parametrize("record", [(690, (11 << 8) | ord("-")), (10, (5 << 8) | ord("A")), (0xFFFFFFF0, (0x20 << 8) | ord("?"))])
def test_bad_records_are_refused(record):
    rows = exception_rows()
    pk = Packed(rows)
    ref = F.random_acgt(NCHAR, 99)
    off = np.array([0] * 5 + [1] * (pk.n - 4), dtype=np.uint64)       # one record, of row 4
    exc = np.array([record], dtype=np.uint32)
    with cluster.Clusterer(ref, dist=DIST) as c:
        with pytest.raises(cluster.ClusterError) as ei:
            c.push_packed(pk.planes, pk.n, off, exc, [0] * pk.n)
        assert ei.value.code == EINVAL
        assert c.stats()["pushed"] == 0                      # nothing was pushed
        with pytest.raises(cluster.ClusterError):
            c.result()                                       # and there is no result
        # the same rows with their own records go through afterwards
        pk.push(c, 0, pk.n, [0] * pk.n)
        c.finish()
        _same((c.result().clusters(), c.result().scores), CL.rs_cluster(ref, rows, [0] * pk.n, DIST, 0, 1, 1))


# ------------------------------------------------------------------------------------------------------------------ command line
def _write_fasta(path, names, seqs):
    with open(path, "wb") as fh:
        for n, s in zip(names, seqs):
            fh.write(b">" + n.encode() + b"\n" + s + b"\n")


def _run(cmd, env=None):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900, env=env)
    assert r.returncode == 0, (cmd, r.stderr[-3000:])
    return r.stderr.decode(errors="replace")


def _xz(path):
    return lzma.open(path, "rb").read()


ARGS = ["-d", "4", "--trim", "100", "-s", "2", "-p", "64"]


@pytest.fixture(scope="module")
def work(tmp_path_factory, bundled):
    names, seqs, _, _ = bundled
    d = tmp_path_factory.mktemp("clust_packed")
    _write_fasta(d / "in.fa", names[:2600], seqs[:2600])
    _run([UVAIAPACK, "-A", "1", "-o", str(d / "in.uvdb"), str(d / "in.fa")])          # -A 1 keeps every record
    env = dict(os.environ, OMP_NUM_THREADS="8")
    _run([UVAIACLUST] + ARGS + ["-o", str(d / "text"), str(d / "in.fa")], env)
    return d, env


def test_cli_packed_writes_the_files_of_the_text_command(work, bundled):
    d, env = work
    names, seqs, _, _ = bundled
    outs = []
    for run in range(2):
        prefix = str(d / ("packed%d" % run))
        err = _run([UVAIACLUST] + ARGS + ["--packed", str(d / "in.uvdb"), "-o", prefix], env)
        assert "decode" in err and "overlay" in err
        outs.append((_xz(prefix + ".csv.xz"), _xz(prefix + ".aln.xz")))
    assert outs[0] == outs[1]                                # two runs, identical files
    assert outs[0] == (_xz(d / "text.csv.xz"), _xz(d / "text.aln.xz"))
    sub_names, sub_seqs = names[:2600], [s.upper() for s in seqs[:2600]]
    ref = CL.rs_reference(sub_seqs[:1024])
    dd, t, s = CL.clamp(len(ref), 4, 100, 2)
    clusters, _ = CL.rs_cluster(ref, sub_seqs, CL.round_robin([2600], 64), dd, t, s, 64)
    assert outs[0][0].decode() == CL.csv_text(clusters, sub_names)
    got = list(zip(*F.read_fasta_bytes(outs[0][1])))
    assert got == CL.aln_records(clusters, sub_names, sub_seqs)


def test_cli_packed_with_a_reference_file(work, bundled):
    d, env = work
    names, seqs, _, _ = bundled
    _write_fasta(d / "ref.fa", [names[100]], [seqs[100]])
    _run([UVAIACLUST] + ARGS + ["-r", str(d / "ref.fa"), "--packed", str(d / "in.uvdb"), "-o", str(d / "packed_r")], env)
    _run([UVAIACLUST] + ARGS + ["-r", str(d / "ref.fa"), "-o", str(d / "text_r"), str(d / "in.fa")], env)
    assert (_xz(d / "packed_r.csv.xz"), _xz(d / "packed_r.aln.xz")) == (_xz(d / "text_r.csv.xz"), _xz(d / "text_r.aln.xz"))


def _n_records(path):
    return len(F.read_fasta_bytes(_xz(path))[0])


def test_packed_out_from_packed_input(work):
    d, env = work
    err = _run([UVAIACLUST] + ARGS + ["--packed", str(d / "in.uvdb"), "--packed-out", str(d / "o1.uvdb"), "-o", str(d / "p1")], env)
    assert "Packed" in err
    assert _xz(d / "p1.aln.xz") == _xz(d / "text.aln.xz") and _xz(d / "p1.csv.xz") == _xz(d / "text.csv.xz")
    _run([UVAIAPACK, "-A", "1", "-o", str(d / "r1.uvdb"), str(d / "p1.aln.xz")])      # the input's recorded value is the default
    assert (d / "o1.uvdb").read_bytes() == (d / "r1.uvdb").read_bytes()


def test_packed_out_from_text_input(work):
    d, env = work
    _run([UVAIACLUST] + ARGS + ["--packed-out", str(d / "o2.uvdb"), "-o", str(d / "p2"), str(d / "in.fa")], env)
    assert _xz(d / "p2.aln.xz") == _xz(d / "text.aln.xz") and _xz(d / "p2.csv.xz") == _xz(d / "text.csv.xz")
    _run([UVAIAPACK, "-o", str(d / "r2.uvdb"), str(d / "p2.aln.xz")])                 # 0.5, the default of both
    assert (d / "o2.uvdb").read_bytes() == (d / "r2.uvdb").read_bytes()


def test_packed_out_with_a_ragged_last_tile(work, bundled):
    d, env = work
    names, seqs, _, _ = bundled
    _write_fasta(d / "small.fa", names[:1000], seqs[:1000])
    _run([UVAIAPACK, "-A", "1", "-o", str(d / "small.uvdb"), str(d / "small.fa")])
    _run([UVAIACLUST, "-d", "2", "-p", "16", "--packed", str(d / "small.uvdb"), "--packed-out", str(d / "o3.uvdb"), "-o", str(d / "p3")], env)
    n = _n_records(d / "p3.aln.xz")
    assert n > 64 and n % 64 != 0
    _run([UVAIAPACK, "-A", "1", "-o", str(d / "r3.uvdb"), str(d / "p3.aln.xz")])
    assert (d / "o3.uvdb").read_bytes() == (d / "r3.uvdb").read_bytes()


def test_packed_out_with_a_filter_that_drops_medoids_and_the_search_over_it(work):
    d, env = work
    names, rows = F.read_fasta_bytes(_xz(d / "text.aln.xz"))
    nchar = len(rows[0])
    counts = sorted(R.count_non_n(r) for r in rows)
    ambig = "%.4f" % (1. - counts[len(counts) // 3] / nchar)                         # about a third of the medoids fall below it
    kept = sum(1 for c in counts if c >= int(nchar * (1. - float(ambig))))
    assert 0 < kept < len(rows)
    err = _run([UVAIACLUST] + ARGS + ["--packed", str(d / "in.uvdb"), "--packed-out", str(d / "o4.uvdb"), "-A", ambig, "-o", str(d / "p4")], env)
    assert "Packed %d of %d medoids" % (kept, len(rows)) in err
    _run([UVAIAPACK, "-A", ambig, "-o", str(d / "r4.uvdb"), str(d / "p4.aln.xz")])
    assert (d / "o4.uvdb").read_bytes() == (d / "r4.uvdb").read_bytes()
    # the searches: the packed medoids answer as their text does
    _write_fasta(d / "queries.fa", ["query %d" % i for i in range(5)], [rows[i] for i in (0, 3, len(rows) // 2, len(rows) - 2, len(rows) - 1)])
    _run([UVAIA, "--packed", str(d / "o4.uvdb"), str(d / "queries.fa"), "-A", ambig, "-n", "6", "-o", str(d / "nn_packed")])
    _run([UVAIA, "-r", str(d / "p4.aln.xz"), str(d / "queries.fa"), "-A", ambig, "-n", "6", "-o", str(d / "nn_text")])
    assert (_xz(d / "nn_packed.csv.xz"), _xz(d / "nn_packed.aln.xz")) == (_xz(d / "nn_text.csv.xz"), _xz(d / "nn_text.aln.xz"))
    assert len(_xz(d / "nn_packed.csv.xz").splitlines()) > 10
