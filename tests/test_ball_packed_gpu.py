"""The radius search over packed tiles that are not resident (uvaia_gpu_ball_packed), text back out of the planes on the device
(uvaia_gpu_unpack_rows) and the command line built on the two (`uvaiaball --packed`), on a GPU box: the same cq->mindist as the text
path and the oracle, the same text as went in, the same .aln.xz as `uvaiaball -r` byte for byte."""
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

import fixtures as F
import oracle_lib as O
import packed_lib as P
from uvaia_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIABALL = os.path.join(ROOT, "bin", "uvaiaball")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")


def _write_fasta(path, names, seqs, opener=open):
    with opener(path, "wb") as fh:
        for n, s in zip(names, seqs):
            fh.write(b">" + n.encode() + b"\n" + s + b"\n")


def _run(cmd, ok=True):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    assert (r.returncode == 0) == ok, (cmd, r.stderr[-2000:])
    return r.stderr.decode(errors="replace")


def _dump(prefix):
    return lzma.open(prefix + ".aln.xz", "rb").read()


def _export_tiles(q_default, refs):
    """the interchange tiles of refs, out of a default-mode context"""
    with capi.Engine.from_query(q_default, nbest=2, max_pool=64) as eng:
        eng.db_reserve(len(refs))
        eng.db_append(refs)
        return eng.db_export()


# ---------------------------------------------------------------------------------------------------------------- API parity
@pytest.mark.parametrize("dist", [0, 3])                     # radii 1 and 4
def test_ball_packed_gives_the_mindist_of_the_text_path_and_of_the_oracle(bundled_db, dist):
    names, seqs = bundled_db
    by = dict(zip(names, seqs))
    qn = F.sample_names_1k()[:12]
    qs = [by[n] for n in qn]
    refs = seqs[:900]                                        # 14 tiles and 4 references of a fifteenth
    planes, _, _ = _export_tiles(O.Query(qs, qn, dist=dist, is_ball=True), refs)
    dirty = planes.copy()
    lanes = dirty.reshape(planes.shape[0], -1, 64, 16)       # [tile][word group x plane][lane][16 bytes]
    lanes[-1, :, len(refs) % 64:, :] = np.random.default_rng(3).integers(0, 256, size=lanes[-1, :, len(refs) % 64:, :].shape, dtype=np.uint8)
    for acgt in (False, True):
        q = O.Query(qs, qn, dist=dist, acgt=acgt, is_ball=True)
        want, _ = q.ball(refs, ambig_r=0.001)                # ambig_r ~ 0: no reference is filtered before scoring
        with capi.Engine.from_query(q, nbest=2, max_pool=512) as eng:
            text = np.concatenate([eng.ball(refs[a:a + 512], q.dist + 1) for a in range(0, len(refs), 512)])
            for tiles in (planes, dirty):
                got = np.concatenate([eng.ball_packed(tiles[a // 64:], min(512, len(refs) - a), q.dist + 1) for a in range(0, len(refs), 512)])
                assert np.array_equal(got, text), (acgt, dist)
                assert np.array_equal(got, want), (acgt, dist)
            assert eng.db_size() == 0                        # the resident database is not touched
            with pytest.raises(capi.GpuError) as ei:         # as uvaia_gpu_ball: a batch above max_pool is refused
                eng.ball_packed(planes, 513, q.dist + 1)
            assert ei.value.code == -6


# ---------------------------------------------------------------------------------------------------------------- unpack
NCHAR = 333                                                  # not a multiple of 32 or 128: the last word is partial


@pytest.fixture(scope="module")
def awkward(tmp_path_factory):
    d = tmp_path_factory.mktemp("unpack")
    root = F.random_acgt(NCHAR, 11)
    qs = []
    for i in range(5):
        s = bytearray(root)
        s[17 * i + 3] = b"ACGT"[(b"ACGT".index(s[17 * i + 3]) + 1) % 4]
        qs.append(bytes(s))
    qn = ["q%d" % i for i in range(len(qs))]
    refs = P.awkward_references(150, NCHAR, seed=23)         # three tiles, 22 references in the last
    upper = [s.upper() for s in refs]
    planes, non_n, side = _export_tiles(O.Query(qs, qn, dist=2, is_ball=True), refs)
    restated, restated_non_n = P.pack_tiles(refs, NCHAR)
    assert np.array_equal(planes, restated) and np.array_equal(non_n, restated_non_n)      # the tiles are what the format says
    names = ["r%d" % i for i in range(len(refs))]
    P.write_uvdb(d / "awkward.uvdb", names, upper, planes, non_n, side)
    return qs, qn, upper, planes, P.Reader(d / "awkward.uvdb", NCHAR)


@pytest.mark.parametrize("acgt", [False, True])
def test_unpack_rows_and_the_exception_pass_give_back_the_text(awkward, acgt):
    qs, qn, upper, planes, reader = awkward
    n = len(upper)
    q = O.Query(qs, qn, dist=2, acgt=acgt, is_ball=True)
    with capi.Engine.from_query(q, nbest=2, max_pool=256) as eng:
        with pytest.raises(capi.GpuError) as ei:             # no batch yet
            eng.unpack_rows([0])
        assert ei.value.code == -6
        md = eng.ball_packed(planes, n, q.dist + 1)
        for index in ([], list(range(n)), list(range(n - 1, -1, -1)), [5, 5, 0, n - 1, 5, 64, 63, 64]):
            rows = eng.unpack_rows(index)
            assert len(rows) == len(index)
            for i, row in zip(index, rows):
                assert row == bytes(ord("N") if c in P.EXCEPTIONS else c for c in upper[i]), (acgt, i)
                assert reader.apply_exceptions(i, row) == upper[i], (acgt, i)
        for bad in ([n], [0, -1], [3, 1 << 20]):             # outside the last batch: an error code, not a fault
            with pytest.raises(capi.GpuError) as ei:
                eng.unpack_rows(bad)
            assert ei.value.code == -1
        assert eng.unpack_rows([n - 1])[0] == P.decode_reference(planes, n - 1, NCHAR)       # ... and the context is still usable
        assert np.array_equal(eng.ball_packed(planes, n, q.dist + 1), md)
        assert np.array_equal(eng.ball_packed(planes, 70, q.dist + 1), md[:70])              # a smaller batch replaces the larger one
        with pytest.raises(capi.GpuError):
            eng.unpack_rows([70])
        assert eng.unpack_rows([69])[0] == P.decode_reference(planes, 69, NCHAR)


# ---------------------------------------------------------------------------------------------------------------- command
@pytest.fixture(scope="module")
def files(tmp_path_factory, bundled_db):
    d = tmp_path_factory.mktemp("ballpacked")
    names, seqs = bundled_db
    by = dict(zip(names, seqs))
    qn = F.sample_names_1k()[:10]
    _write_fasta(d / "query.fa", qn, [by[n] for n in qn])
    far = []                                                 # queries a thousand substitutions away from everything: nothing is kept
    for n in qn[:3]:
        s = bytearray(by[n])
        for pos in range(300, len(s) - 300, 25):
            if s[pos] in b"ACGT":
                s[pos] = b"ACGT"[(b"ACGT".index(s[pos]) + 1) % 4]
        far.append(bytes(s))
    _write_fasta(d / "far.fa", ["far%d" % i for i in range(3)], far)
    _write_fasta(d / "ref1.aln.xz", names[:1200], seqs[:1200], opener=lzma.open)
    _write_fasta(d / "ref2.fa", names[1200:1500], seqs[1200:1500])
    _run([UVAIAPACK, "-o", str(d / "refs.uvdb"), str(d / "ref1.aln.xz"), str(d / "ref2.fa")])
    return d, qn, [by[n] for n in qn], names[:1500], seqs[:1500]


@pytest.mark.parametrize("query,extra,packed_only", [
    ("query.fa", [], []),
    ("query.fa", ["--acgt"], []),
    ("query.fa", ["--trim", "230", "-k"], []),
    ("query.fa", ["-d", "0"], []),
    ("query.fa", ["-d", "10"], []),
    ("query.fa", ["-d", "200"], []),                         # keeps nearly everything
    ("query.fa", ["-p", "100"], []),                         # chunks of 64: many of them, the last one partial
    ("query.fa", ["-p", "256"], ["--devices", "0,0"]),       # two contexts on one GPU, three chunks each
    ("far.fa", ["-d", "0"], []),                             # keeps nothing
])
def test_uvaiaball_packed_writes_the_file_of_the_text_path(files, query, extra, packed_only):
    d, qn, qs, rnames, rseqs = files
    tag = "_".join(x.strip("-").replace(",", "") for x in [query[:3]] + extra + packed_only)
    out_t, out_p = str(d / ("t_" + tag)), str(d / ("p_" + tag))
    _run([UVAIABALL, "-r", str(d / "ref1.aln.xz"), "-r", str(d / "ref2.fa"), str(d / query), "-o", out_t] + extra)
    log = _run([UVAIABALL, "--packed", str(d / "refs.uvdb"), str(d / query), "-o", out_p] + extra + packed_only)
    text, packed = _dump(out_t), _dump(out_p)
    assert packed == text
    n_db = int(re.search(r"Loaded (\d+) packed sequences", log).group(1))
    kept = packed.count(b">")
    assert int(re.search(r"Saved (\d+) sequences", log).group(1)) == kept
    if "-p" in extra:
        chunk = int(extra[extra.index("-p") + 1]) // 64 * 64
        assert n_db > 3 * chunk and ("--devices" in packed_only or n_db % chunk != 0)
    if extra == ["-d", "200"]:
        assert kept > 0.9 * n_db
    if query == "far.fa":
        assert kept == 0 and text == b""
    elif extra != ["-d", "0"]:
        assert kept > 0
    if not extra:                                            # the default case against the oracle as well
        q = O.Query(qs, qn, dist=1, is_ball=True)
        _, keep = q.ball(rseqs, ambig_r=0.5)
        got_names, got_seqs = F.read_fasta_bytes(packed)
        assert got_names == [rnames[i] for i in np.nonzero(keep)[0]]
        assert got_seqs == [rseqs[i] for i in np.nonzero(keep)[0]]


def test_uvaiaball_packed_applies_its_own_filter_or_refuses(tmp_path):
    """Packed with -A 0.5 a file of 400 sites holds the references with at least 200 valid sites.  -A 0.7 (280) can be answered from
    it and drops the reference with 240; -A 0.3 (120) cannot: the reference with 150 valid sites is not in the file."""
    nchar = 400
    root = F.random_acgt(nchar, 5)

    def variant(positions, n_from=0, n_len=0):
        s = bytearray(root)
        for pos in positions:
            s[pos] = b"ACGT"[(b"ACGT".index(s[pos]) + 1) % 4]
        s[n_from:n_from + n_len] = b"N" * n_len
        return bytes(s)

    qs = [variant([10 * i + 1]) for i in range(3)]
    refs = [variant([7 * i + 2, 11 * i + 5][:i % 3]) for i in range(20)] + [variant([], 100, 160), variant([], 100, 250), variant([3], 50, 100)]
    rn = ["r%d" % i for i in range(20)] + ["valid240", "valid150", "valid300"]
    _write_fasta(tmp_path / "q.fa", ["q0", "q1", "q2"], qs)
    _write_fasta(tmp_path / "r.fa", rn, refs)
    db = str(tmp_path / "r.uvdb")
    _run([UVAIAPACK, "-A", "0.5", "-o", db, str(tmp_path / "r.fa")])
    kept = {}
    for a in ("0.5", "0.7"):
        out_t, out_p = str(tmp_path / ("t" + a)), str(tmp_path / ("p" + a))
        _run([UVAIABALL, "-r", str(tmp_path / "r.fa"), str(tmp_path / "q.fa"), "-d", "5", "-A", a, "-o", out_t])
        _run([UVAIABALL, "--packed", db, str(tmp_path / "q.fa"), "-d", "5", "-A", a, "-o", out_p])
        assert _dump(out_p) == _dump(out_t)
        kept[a] = F.read_fasta_bytes(_dump(out_p))[0]
    assert "valid240" in kept["0.5"] and "valid240" not in kept["0.7"]          # dropped by the filter, not by the radius
    assert "valid300" in kept["0.7"] and "valid150" not in kept["0.5"]
    log = _run([UVAIABALL, "--packed", db, str(tmp_path / "q.fa"), "-A", "0.3", "-o", str(tmp_path / "refused")], ok=False)
    assert "packed" in log
    _run([UVAIABALL, "--packed", db, "-r", str(tmp_path / "r.fa"), str(tmp_path / "q.fa"), "-o", str(tmp_path / "both")], ok=False)
    _run([UVAIABALL, str(tmp_path / "q.fa"), "-o", str(tmp_path / "neither")], ok=False)
