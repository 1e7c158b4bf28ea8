"""`uvaiadist -d D --clusters` end to end on the constructed chains (260 sequences of 513 sites): the cluster lines equal, byte for byte,
the text built from the restatement of pair_link.py, whatever the input (FASTA, a dense, a compact packed database) and however the
rows are cut into bands; the options of the form; its report; and the forms that existed before write what they wrote."""
import json
import os
import subprocess

import numpy as np
import pytest

import pair_dist as D
import pair_link as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


def run(tool, *args):
    r = subprocess.run([os.path.join(BIN, tool), *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    return r


def dist(*args):
    return run("uvaiadist", "--stdout", *args)


def report(r):
    line = [l for l in r.stderr.decode().splitlines() if l.startswith("dist report: ")]
    assert len(line) == 1
    return json.loads(line[0][len("dist report: "):])


class Inputs:
    pass


def write_inputs(d, stem, names, seqs):
    fasta, dense, compact = d / (stem + ".fa"), d / (stem + ".uvdb"), d / (stem + ".compact.uvdb")
    fasta.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    run("uvaiapack", "-A", 1, "-o", dense, fasta)
    run("uvaiapack", "-A", 1, "--compact", "-o", compact, fasta)
    return fasta, dense, compact


@pytest.fixture(scope="module")
def inp(tmp_path_factory):
    d = tmp_path_factory.mktemp("uvaiadist_clusters")
    x = Inputs()
    x.seqs, _nchar = K.case("chains260x513")
    x.names = ["chain_%03d" % i for i in range(len(x.seqs))]
    x.counts = K.counts("chains260x513")
    x.fasta, x.dense, x.compact = write_inputs(d, "chains", x.names, x.seqs)
    x.sp_seqs, _nchar = K.case("special129")
    x.sp_names = ["all_N", "all_gap", "partial", "a", "a_again", "b"]
    x.sp_fasta, x.sp_dense, _ = write_inputs(d, "special", x.sp_names, x.sp_seqs)
    return x


def test_every_kind_of_input_gives_the_same_bytes(inp):
    labels, links = K.restate(inp.counts, "snp", 1)
    want = K.clusters_text(inp.names, labels)
    assert want.count(b"\n") == 260 and want.startswith(b"chain_000\t1\t")
    for source in (("--packed", inp.dense), ("--packed", inp.compact), (inp.fasta,)):
        r = dist("-d", 1, "--clusters", *source)
        assert r.stdout == want, source
        rep = report(r)
        assert (rep["sequences"], rep["links"], rep["clusters"], rep["largest"], rep["bands"]) == (260, links, 8, 65, 1) and links == 252
        assert "pairs" not in rep and rep["kernel_ms"] > 0
    assert dist("-d", 1, "--clusters", "--metric=uvaia", "--packed", inp.dense).stdout == K.clusters_text(inp.names, K.restate(inp.counts, "uvaia", 1)[0])
    assert dist("-d", 0, "--clusters", "--packed", inp.dense).stdout == K.clusters_text(inp.names, np.arange(260))
    assert dist("-d", 64, "--clusters", "--packed", inp.dense).stdout == K.clusters_text(inp.names, np.zeros(260, dtype=np.uint32))


def test_bands_of_rows_give_the_same_bytes(inp):
    labels, links = K.restate(inp.counts, "snp", 1)
    r = dist("-d", 1, "--clusters", "--band-rows", 64, "--packed", inp.dense)
    assert r.stdout == K.clusters_text(inp.names, labels)
    rep = report(r)
    assert (rep["links"], rep["clusters"], rep["largest"], rep["bands"]) == (links, 8, 65, 5)


def test_csv_and_min_size(inp):
    labels, _links = K.restate(inp.counts, "snp", 1)
    assert dist("-d", 1, "--clusters", "--csv", "--packed", inp.dense).stdout == K.clusters_text(inp.names, labels, sep=",")
    want = K.clusters_text(inp.names, labels, min_size=2)
    assert want.count(b"\n") == 258                    # the two singleton families are left out, the numbering is that of the full text
    r = dist("-d", 1, "--clusters", "--min-size", 2, "--packed", inp.dense)
    assert r.stdout == want and report(r)["clusters"] == 8
    assert dist("-d", 1, "--clusters", "--min-size", 64, "--packed", inp.dense).stdout == K.clusters_text(inp.names, labels, min_size=64)
    assert dist("-d", 1, "--clusters", "--min-size", 66, "--packed", inp.dense).stdout == b""
    out = inp.dense.parent / "clusters.tsv"
    run("uvaiadist", "-d", 1, "--clusters", "-o", out, "--packed", inp.dense)
    assert out.read_bytes() == K.clusters_text(inp.names, labels)


def test_min_compared(inp):
    """under snp the all-N row joins everything; --min-compared 1 is what is set against it"""
    c = K.counts("special129")
    r = dist("-d", 0, "--clusters", "--packed", inp.sp_dense)
    assert r.stdout == K.clusters_text(inp.sp_names, K.restate(c, "snp", 0)[0]) == b"".join(b"%s\t1\t6\n" % n.encode() for n in inp.sp_names)
    for source in (("--packed", inp.sp_dense), (inp.sp_fasta,)):
        r = dist("-d", 0, "--clusters", "--min-compared", 1, *source)
        assert r.stdout == K.clusters_text(inp.sp_names, K.restate(c, "snp", 0, 1)[0]) == b"all_N\t1\t1\nall_gap\t2\t1\npartial\t3\t1\na\t4\t2\na_again\t4\t2\nb\t5\t1\n"
        assert (report(r)["links"], report(r)["clusters"], report(r)["largest"]) == (1, 5, 2)
    for floor in (129, 130):
        got = dist("-d", 0, "--clusters", "--metric=uvaia", "--min-compared", floor, "--packed", inp.sp_dense).stdout
        assert got == K.clusters_text(inp.sp_names, K.restate(c, "uvaia", 0, floor)[0])
    labels = K.restate(inp.counts, "snp", 1, 514)[0]
    assert np.array_equal(labels, np.arange(260))
    assert dist("-d", 1, "--clusters", "--min-compared", 514, "--packed", inp.dense).stdout == K.clusters_text(inp.names, labels)
    assert dist("-d", 1, "--clusters", "--min-compared", 513, "--packed", inp.dense).stdout == K.clusters_text(inp.names, K.restate(inp.counts, "snp", 1)[0])


def test_trim(inp):
    c = D.oracle_counts_of(inp.seqs, 100)
    labels = K.restate(c, "snp", 0)[0]
    assert 8 < len(set(labels.tolist())) < 260         # rows that differ only outside the window are identical inside it
    assert dist("-d", 0, "--clusters", "--trim", 100, "--packed", inp.dense).stdout == K.clusters_text(inp.names, labels)


# ---- the forms that existed before: text built here from the oracle's counters, as test_uvaiadist_cli_gpu.py builds it
def test_the_other_forms_write_what_they_wrote(inp):
    d = D.snp(inp.counts)
    lines = ["%s,%s,%d\n" % (inp.names[i], inp.names[j], d[i, j]) for i in range(260) for j in range(i + 1, 260) if d[i, j] <= 1]
    assert len(lines) == 252
    r = dist("-d", 1, "--packed", inp.dense)
    assert r.stdout == "".join(lines).encode()
    assert r.stderr.decode().splitlines()[-1].startswith('dist report: {"sequences": 260, "pairs": 252, "bands": 1, "load_ms": ')
    assert set(report(r)) == {"sequences", "pairs", "bands", "load_ms", "kernel_ms", "format_ms", "write_ms"}
    table = ["\t".join(["uvaiadist"] + inp.names)] + ["\t".join([n] + [str(int(v)) for v in row]) for n, row in zip(inp.names, d)]
    r = dist("--packed", inp.dense)
    assert r.stdout == ("\n".join(table) + "\n").encode()
    assert b'"sequences": 260, "pairs": 67600, "bands": 1,' in r.stderr
