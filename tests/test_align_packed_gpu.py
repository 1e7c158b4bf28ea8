"""`uvaialign --packed` on a GPU box: the database it writes is, byte for byte, the one `uvaialign -o` + `uvaiapack` write, whatever the pool
size; the text output next to it is what it is without --packed; `uvaia --packed` answers the same over both files."""
import lzma
import os
import subprocess

import numpy as np
import pytest

import fixtures as F
import rows_lib as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIA = os.path.join(ROOT, "bin", "uvaia")
UVAIALIGN = os.path.join(ROOT, "bin", "uvaialign")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")
AMBIG_R = "0.2"


def _write_fasta(path, names, seqs, opener=open):
    with opener(path, "wb") as fh:
        for n, s in zip(names, seqs):
            fh.write(b">" + n.encode() + b"\n" + s + b"\n")


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, (cmd, r.stderr[-3000:])
    return r.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """one reference, 330 unaligned sequences: SNPs, insertions and deletions throughout; every seventh is N-rich (it passes the aligner's
    -a 0.5 and fails -A 0.2), some hold runs of '?', 'X' and '.'; what is kept spans more than four tiles and ends inside one"""
    d = tmp_path_factory.mktemp("align_packed")
    ref = F.random_acgt(2003, 31)
    seqs = F.unaligned_queries(ref, 330, 32, p_indel=0.0015, n_runs=(30, 30, 100))
    rng = np.random.default_rng(33)
    out = []
    for i, s in enumerate(seqs):
        s = bytearray(s)
        if i % 7 == 3:                                                   # 30 % N: kept by the aligner, dropped by -A 0.2
            a = int(rng.integers(0, len(s) // 2))
            k = (3 * len(s)) // 10
            s[a:a + k] = b"N" * k
        if i % 11 == 5:
            for ch in b"?X.":
                a, k = int(rng.integers(0, len(s) - 12)), int(rng.integers(1, 12))
                s[a:a + k] = bytes([ch]) * k
        out.append(bytes(s))
    names = ["hCoV-19/seq %d|2021-0%d" % (i, 1 + i % 9) for i in range(len(out))]
    _write_fasta(d / "ref.fa", ["the reference"], [ref])
    _write_fasta(d / "raw1.fa", names[:200], out[:200])
    _write_fasta(d / "raw2.fa.xz", names[200:], out[200:], opener=lzma.open)      # two input files: pools end with a file
    # the two-step way: text, then uvaiapack
    _run([UVAIALIGN, "-r", str(d / "ref.fa"), str(d / "raw1.fa"), str(d / "raw2.fa.xz"), "-o", str(d / "t"), "-p", "64"])
    _run([UVAIAPACK, "-A", AMBIG_R, "-o", str(d / "b.uvdb"), str(d / "t.aln.xz")])
    return d, ref


def _packed(d, tag, extra):
    path = d / ("a_%s.uvdb" % tag)
    err = _run([UVAIALIGN, "-r", str(d / "ref.fa"), str(d / "raw1.fa"), str(d / "raw2.fa.xz"), "--packed", str(path), "-A", AMBIG_R] + extra)
    return path, err


def test_the_input_covers_what_it_should(work):
    d, ref = work
    names, rows = F.read_fasta_bytes(lzma.open(d / "t.aln.xz", "rb").read())
    assert len(rows) >= 300 and all(len(r) == len(ref) for r in rows)
    kept = [r for r in rows if R.count_non_n(r) >= int(len(ref) * (1 - float(AMBIG_R)))]
    assert len(kept) > 4 * 64 and len(kept) % 64 != 0 and len(rows) - len(kept) >= 20
    assert sum(1 for r in kept if b"-" in r) > 100                       # deletions
    for ch in (b"?", b"X", b"."):
        assert any(ch in r for r in kept)


@pytest.mark.parametrize("pool", [37, 64, 100000])
def test_packed_database_is_the_file_uvaiapack_writes_whatever_the_pool(work, pool):
    d, _ = work
    path, err = _packed(d, "p%d" % pool, ["-p", str(pool)])
    assert path.read_bytes() == (d / "b.uvdb").read_bytes()
    assert "Packed" in err


def test_default_pool_and_default_ambiguity(work):
    d, _ = work
    _run([UVAIAPACK, "-o", str(d / "b_default.uvdb"), str(d / "t.aln.xz")])
    before = set(os.listdir(os.getcwd()))
    _run([UVAIALIGN, "-r", str(d / "ref.fa"), str(d / "raw1.fa"), str(d / "raw2.fa.xz"), "--packed", str(d / "a_default.uvdb")])
    assert (d / "a_default.uvdb").read_bytes() == (d / "b_default.uvdb").read_bytes()
    assert set(os.listdir(os.getcwd())) == before                       # and no text file of a made-up name


def test_text_next_to_the_database_is_todays_text(work):
    d, _ = work
    path, _ = _packed(d, "with_text", ["-p", "50", "-o", str(d / "t2")])
    assert path.read_bytes() == (d / "b.uvdb").read_bytes()
    assert lzma.open(d / "t2.aln.xz", "rb").read() == lzma.open(d / "t.aln.xz", "rb").read()
    r = subprocess.run([UVAIALIGN, "-r", str(d / "ref.fa"), str(d / "raw1.fa"), str(d / "raw2.fa.xz"), "--packed", str(d / "a_stdout.uvdb"), "-A", AMBIG_R, "--stdout"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == lzma.open(d / "t.aln.xz", "rb").read()
    assert (d / "a_stdout.uvdb").read_bytes() == (d / "b.uvdb").read_bytes()


def test_search_over_both_databases_gives_the_same_table(work):
    d, ref = work
    path, _ = _packed(d, "search", ["-p", "200"])
    names, rows = F.read_fasta_bytes(lzma.open(d / "t.aln.xz", "rb").read())
    _write_fasta(d / "queries.fa", ["query %d" % i for i in range(6)], [rows[i] for i in (0, 9, 50, 120, 250, 300)])
    tables = []
    for tag, db in (("a", path), ("b", d / "b.uvdb")):
        out = str(d / ("nn_" + tag))
        _run([UVAIA, "--packed", str(db), str(d / "queries.fa"), "-A", AMBIG_R, "-n", "6", "-o", out])
        tables.append((lzma.open(out + ".csv.xz", "rb").read(), lzma.open(out + ".aln.xz", "rb").read()))
    assert tables[0] == tables[1]
    assert len(tables[0][0].splitlines()) > 12


def test_a_sequence_the_engine_refuses_ends_the_command_with_both_files_closed(work):
    d, ref = work
    seqs = F.unaligned_queries(ref, 90, 77, n_runs=(0, 0, 0))
    bad = bytearray(seqs[70]); bad[500] = ord("U"); seqs[70] = bytes(bad)            # RNA: outside the engine's alphabet
    _write_fasta(d / "bad.fa", ["s%d" % i for i in range(len(seqs))], seqs)
    r = subprocess.run([UVAIALIGN, "-r", str(d / "ref.fa"), str(d / "bad.fa"), "--packed", str(d / "bad.uvdb"), "-p", "32", "-o", str(d / "bad_t")],
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode != 0
    assert b"packing pool 3" in r.stderr and b"s64" in r.stderr
    import packed_lib as P
    rd = P.Reader(d / "bad.uvdb", len(ref))                              # a complete file of the 64 sequences of the first two pools
    assert rd.unpack_reference(63)
    rd.close()
    names, rows = F.read_fasta_bytes(lzma.open(d / "bad_t.aln.xz", "rb").read())
    assert names == ["s%d" % i for i in range(64)]
