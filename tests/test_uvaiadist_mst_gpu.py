"""`uvaiadist --mst` and `--nearest` end to end: the text equals, byte for byte, the text built from the restatement of pair_mst.py, whatever
the input (a dense or compact packed database, two databases as one stream, aligned FASTA) and whatever the options that go with the
forms; the report line; every refused combination; and `--min-compared` on its own is still refused as it was."""
import json
import os
import subprocess

import numpy as np
import pytest

import pair_dist as D
import pair_link as K
import pair_mst as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


def run(tool, *args, ok=True):
    r = subprocess.run([os.path.join(BIN, tool), *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr.decode()
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
    d = tmp_path_factory.mktemp("uvaiadist_mst")
    x = Inputs()
    x.dir = d
    x.seqs, _nchar = M.case("synth130")
    x.names = ["synth_%03d" % i for i in range(len(x.seqs))]
    x.counts = M.counts("synth130")
    x.fasta, x.dense, x.compact = write_inputs(d, "synth", x.names, x.seqs)
    _f, x.head, _c = write_inputs(d, "head", x.names[:70], x.seqs[:70])       # the same rows as two databases
    _f, x.tail, _c = write_inputs(d, "tail", x.names[70:], x.seqs[70:])
    x.sp_seqs, _nchar = M.case("special129")
    x.sp_names = ["all_N", "all_gap", "partial", "a", "a_again", "b"]
    x.sp_counts = M.counts("special129")
    x.sp_fasta, x.sp_dense, _ = write_inputs(d, "special", x.sp_names, x.sp_seqs)
    return x


def texts(names, counts, metric="snp", floor=0, sep="\t"):
    return {"--mst": M.mst_text(names, M.kruskal(counts, metric, floor), sep), "--nearest": M.nearest_text(names, M.nearest(counts, metric, floor), sep)}


@pytest.mark.parametrize("form", ["--mst", "--nearest"])
def test_every_kind_of_input_gives_the_same_bytes(inp, form):
    want = texts(inp.names, inp.counts)[form]
    assert want.count(b"\n") == (129 if form == "--mst" else 130)
    for source in (("--packed", inp.dense), ("--packed", inp.compact), ("--packed", inp.head, "--packed", inp.tail), (inp.fasta,)):
        assert dist(form, *source).stdout == want, source


@pytest.mark.parametrize("form", ["--mst", "--nearest"])
def test_the_options_that_go_with_the_forms(inp, form):
    src = ("--packed", inp.dense)
    assert dist(form, "--csv", *src).stdout == texts(inp.names, inp.counts, sep=",")[form]
    assert dist(form, "--metric=uvaia", *src).stdout == texts(inp.names, inp.counts, "uvaia")[form]
    assert dist(form, "--trim", 33, *src).stdout == texts(inp.names, M.counts("synth130", 33))[form]
    want = texts(inp.names, inp.counts, floor=K.SYNTH_FLOOR)[form]
    assert want != texts(inp.names, inp.counts)[form]
    assert dist(form, "--min-compared", K.SYNTH_FLOOR, *src).stdout == want


@pytest.mark.parametrize("form", ["--mst", "--nearest"])
def test_where_the_text_goes(inp, form):
    src = ("--packed", inp.dense)
    assert dist(form, "--band-rows", 40, "-A", 1, *src).stdout == texts(inp.names, inp.counts)[form]
    out = inp.dir / ("out%s.tsv" % form)
    run("uvaiadist", form, "-o", out, *src)
    assert out.read_bytes() == texts(inp.names, inp.counts)[form]
    out = inp.dir / ("out%s.tsv.gz" % form)
    run("uvaiadist", form, "-o", out, *src)
    assert subprocess.run(["gzip", "-dc", str(out)], stdout=subprocess.PIPE, check=True).stdout == texts(inp.names, inp.counts)[form]


def test_the_hub_the_floor_and_the_row_without_a_partner(inp):
    src = ("--packed", inp.sp_dense)
    assert dist("--mst", *src).stdout == b"".join(b"all_N\t%s\t0\n" % n.encode() for n in inp.sp_names[1:])
    assert dist("--nearest", *src).stdout == b"all_N\tall_gap\t0\n" + b"".join(b"%s\tall_N\t0\n" % n.encode() for n in inp.sp_names[1:])
    for source in (src, (inp.sp_fasta,)):
        r = dist("--mst", "--min-compared", 1, *source)
        assert r.stdout == texts(inp.sp_names, inp.sp_counts, floor=1)["--mst"] and r.stdout.startswith(b"a\ta_again\t0\n")
        rep = report(r)
        assert (rep["sequences"], rep["edges"], rep["trees"]) == (6, 2, 4)
        r = dist("--nearest", "--min-compared", 1, "--csv", *source)
        assert r.stdout == texts(inp.sp_names, inp.sp_counts, floor=1, sep=",")["--nearest"] and r.stdout.startswith(b"all_N,,-1\nall_gap,,-1\npartial,,-1\na,a_again,0\n")


def test_the_report_line(inp):
    edges = M.kruskal(inp.counts, "snp")
    r = dist("--mst", "--packed", inp.dense)
    rep = report(r)
    assert list(rep) == ["sequences", "edges", "trees", "rounds", "weight", "tiles_walked", "tiles_skipped", "load_ms", "kernel_ms", "format_ms", "write_ms"]
    assert (rep["sequences"], rep["edges"], rep["trees"], rep["weight"]) == (130, 129, 1, sum(d for _a, _b, d in edges))
    assert 1 <= rep["rounds"] <= 9 and rep["tiles_walked"] > 0 and rep["kernel_ms"] > 0
    assert b"minimum spanning tree of 130 of 130 sequences" in r.stderr
    edges = M.kruskal(inp.counts, "uvaia", K.SYNTH_FLOOR)
    rep = report(dist("--mst", "--metric=uvaia", "--min-compared", K.SYNTH_FLOOR, "--packed", inp.dense))
    assert (rep["edges"], rep["trees"], rep["weight"]) == (len(edges), 130 - len(edges), sum(d for _a, _b, d in edges)) and rep["trees"] > 1
    best = M.nearest(inp.counts, "snp")
    rep = report(dist("--nearest", "--packed", inp.dense))
    assert (rep["sequences"], rep["nearest"], rep["rounds"], rep["weight"]) == (130, 130, 1, sum(int(b) >> 32 for b in best))
    assert rep["tiles_walked"] == M.tile_stats(np.arange(130), "snp")[0] and rep["tiles_skipped"] == 0


@pytest.mark.parametrize("form", ["--mst", "--nearest"])
def test_refused_combinations(inp, form):
    for args, message in ((("-d", 1), "does not go with -d"), (("--clusters",), "does not go with --clusters"), (("-d", 1, "--clusters"), "does not go with -d"),
                          (("--long",), "does not go with --long"), (("--counts",), "does not go with --counts"), (("--dense",), "does not go with --dense"),
                          (("--min-size", 2), "does not go with --min-size")):
        r = run("uvaiadist", form, *args, "--stdout", "--packed", inp.dense, ok=False)
        assert ("%s %s" % (form, message)).encode() in r.stderr and not r.stdout, args
    r = run("uvaiadist", "--mst", "--nearest", "--stdout", "--packed", inp.dense, ok=False)
    assert b"--mst and --nearest are two forms of the output: give one" in r.stderr and not r.stdout
    r = run("uvaiadist", form, "--trim", 300, "--stdout", "--packed", inp.dense, ok=False)
    assert b"--trim 300 on both sides leaves nothing of 513 sites" in r.stderr


def test_min_compared_alone_is_refused_as_before(inp):
    r = run("uvaiadist", "--min-compared", 5, "--stdout", "--packed", inp.dense, ok=False)
    assert r.stderr == b"--min-compared needs --clusters: it decides which pairs link two sequences\n" and not r.stdout
    r = run("uvaiadist", "-d", 1, "--min-compared", 5, "--stdout", "--packed", inp.dense, ok=False)
    assert r.stderr == b"--min-compared needs --clusters: it decides which pairs link two sequences\n"
    d = D.snp(inp.counts)
    table = ["\t".join(["uvaiadist"] + inp.names)] + ["\t".join([n] + [str(int(v)) for v in row]) for n, row in zip(inp.names, d)]
    assert dist("--packed", inp.dense).stdout == ("\n".join(table) + "\n").encode()       # the table is what it was
