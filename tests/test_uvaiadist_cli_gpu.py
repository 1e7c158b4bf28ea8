"""`uvaiadist` end to end on 150 sequences of the bundled alignment (29 903 columns, --trim 230): every form of the output equals the text
built here from the oracle's counters, whatever the input is (FASTA, a dense, a compact, two packed databases) and however the matrix is
cut into bands."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fixtures as F
import pair_dist as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
TRIM, N = 230, 150
COUNTS_HEADER = "a,b,ACGT_matches,text_matches,partial_matches,valid_pair_comparisons,ACGT_pair_comparisons,snp_distance\n"


def run(tool, *args):
    r = subprocess.run([os.path.join(BIN, tool), *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    return r


class Inputs:
    pass


@pytest.fixture(scope="module")
def inp(tmp_path_factory):
    d = tmp_path_factory.mktemp("uvaiadist")
    names, seqs = F.load_bundled()
    x = Inputs()
    x.dir = d
    x.names, x.seqs = names[::61][:N], seqs[::61][:N]          # a sample with good and poor rows (7 of them pass -A 0.01)
    assert len(x.names) == N and len(set(x.names)) == N
    x.counts = D.oracle_counts_of(x.seqs, TRIM)
    x.fasta = d / "aln.fa"
    x.fasta.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(x.names, x.seqs)))
    parts = [d / "a.fa", d / "b.fa"]
    parts[0].write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(x.names[:80], x.seqs[:80])))
    parts[1].write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(x.names[80:], x.seqs[80:])))
    x.dense, x.compact, x.two = d / "dense.uvdb", d / "compact.uvdb", [d / "a.uvdb", d / "b.uvdb"]
    run("uvaiapack", "-A", 1, "-o", x.dense, x.fasta)
    run("uvaiapack", "-A", 1, "--compact", "-o", x.compact, x.fasta)
    for p, o in zip(parts, x.two):
        run("uvaiapack", "-A", 1, "-o", o, p)
    return x


def table(names, dist, sep="\t"):
    out = [sep.join(["uvaiadist"] + list(names))]
    for n, row in zip(names, dist):
        out.append(sep.join([n] + [str(int(v)) for v in row]))
    return ("\n".join(out) + "\n").encode()


def long_lines(names, counts, metric, keep=None, with_counts=False):
    d = D.snp(counts) if metric == "snp" else D.uvaia(counts)
    out = [COUNTS_HEADER] if with_counts else []
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            if keep is not None and d[i, j] > keep:
                continue
            if with_counts:
                out.append("%s,%s,%s,%d\n" % (names[i], names[j], ",".join(str(int(v)) for v in counts[i, j]), D.snp(counts)[i, j]))
            else:
                out.append("%s,%s,%d\n" % (names[i], names[j], d[i, j]))
    return "".join(out).encode()


def dist(*args):
    return run("uvaiadist", "--trim", TRIM, "--stdout", *args)


@pytest.mark.parametrize("metric", ["snp", "uvaia"])
def test_dense_table(inp, metric):
    d = D.snp(inp.counts) if metric == "snp" else D.uvaia(inp.counts)
    want = table(inp.names, d)
    r = dist("--metric=" + metric, inp.fasta)
    assert r.stdout == want
    assert b"dist report: {" in r.stderr and b'"sequences": 150' in r.stderr and b'"pairs": 22500' in r.stderr and b'"bands": 1,' in r.stderr
    r = dist("--metric=" + metric, "--band-rows", 64, inp.fasta)
    assert r.stdout == want and b'"bands": 3,' in r.stderr


def test_csv_and_compressed_output(inp):
    want = table(inp.names, D.snp(inp.counts), sep=",")
    assert dist("--csv", "--packed", inp.dense).stdout == want
    out = inp.dir / "table.csv.gz"
    run("uvaiadist", "--trim", TRIM, "--csv", "-o", out, "--packed", inp.dense)
    assert gzip.open(out, "rb").read() == want


@pytest.mark.parametrize("metric", ["snp", "uvaia"])
def test_long_forms(inp, metric):
    assert dist("--metric=" + metric, "--long", "--band-rows", 64, "--packed", inp.dense).stdout == long_lines(inp.names, inp.counts, metric)
    assert dist("--metric=" + metric, "--counts", "--packed", inp.dense).stdout == long_lines(inp.names, inp.counts, metric, with_counts=True)


@pytest.mark.parametrize("metric", ["snp", "uvaia"])
def test_pairs_within_a_distance(inp, metric):
    want = long_lines(inp.names, inp.counts, metric, keep=2)
    assert want.count(b"\n") == 597
    r = dist("--metric=" + metric, "-d", 2, "--band-rows", 64, "--list-cap", 16, "--packed", inp.dense)     # the list has to grow in every band
    assert r.stdout == want and b'"pairs": 597,' in r.stderr and b'"bands": 3,' in r.stderr
    assert dist("--metric=" + metric, "-d", 2, "--counts", "--packed", inp.dense).stdout == long_lines(inp.names, inp.counts, metric, keep=2, with_counts=True)


def test_every_kind_of_input_gives_the_same_bytes(inp):
    want = table(inp.names, D.snp(inp.counts))
    assert dist("--packed", inp.dense).stdout == want
    assert dist("--packed", inp.compact).stdout == want
    assert dist("--packed", inp.two[0], "--packed", inp.two[1]).stdout == want
    assert dist(inp.dir / "a.fa", inp.dir / "b.fa").stdout == want


def test_ambiguity_filter_drops_the_rows_it_should(inp):
    thr = int(29903 * (1 - 0.01))
    invalid = np.zeros(256, dtype=bool)
    invalid[list(b"NX-?O.")] = True
    keep = [i for i, s in enumerate(inp.seqs) if int((~invalid[np.frombuffer(s, dtype=np.uint8)]).sum()) >= thr]
    assert len(keep) == 7
    want = table([inp.names[i] for i in keep], D.snp(inp.counts)[np.ix_(keep, keep)])
    for source in (("--packed", inp.dense), (inp.fasta,)):
        r = dist("-A", 0.01, *source)
        assert r.stdout == want and b"7 of 150 sequences" in r.stderr


def test_a_sequence_of_another_length_is_named(inp):
    bad = inp.dir / "bad.fa"
    bad.write_bytes(b">first\nACGTACGT\n>the_short_one\nACGTAC\n")
    r = subprocess.run([os.path.join(BIN, "uvaiadist"), "--stdout", str(bad)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0 and b"the_short_one" in r.stderr
