"""`uvaia -r --device-parse` and `uvaiaclust --device-parse` on a GPU box: the commands write what they write without the option -- the
same table, the same alignments, the same totals -- whatever the block size and the window, from plain, wrapped and compressed FASTA."""
import filecmp
import gzip
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

import fasta_lib as FL
import fixtures as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIA = os.path.join(ROOT, "bin", "uvaia")
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")
NCHAR, POOL = 600, 64


def _run_together(cmds):
    """[(return code, stderr)] of the commands, ten at a time"""
    out = []
    for a in range(0, len(cmds), 10):
        procs = [subprocess.Popen(c, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE) for c in cmds[a:a + 10]]
        try:
            for p in procs:
                err = p.communicate(timeout=600)[1]
                out.append((p.returncode, err.decode(errors="replace")))
        finally:                                               # a timeout (or any other way out) leaves none of the batch running
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.communicate()
        died = [(c, r) for c, r in zip(cmds[a:a + 10], out[a:]) if r[0] < 0 or r[0] in (124, 134, 137, 139)]
        assert not died, died[:2]                              # a command that was killed: nothing more is started
    return out


def _references():
    """(names, sequences, first file's records, accepted of the first file at -A 0.9): some 300 relatives of one root with everything the
    fill loop filters on"""
    refs, root, cols = F.synth_alignment(300, NCHAR, seed=31, p_snp=0.02, p_amb=0.003)
    names = [b"r%d" % i for i in range(300)]
    rng = np.random.default_rng(33)
    for i in range(300):
        s = bytearray(refs[i])
        if i % 11 == 2:                                        # the exception characters of a packed database
            for ch in b"-?XO.":
                a, k = int(rng.integers(0, NCHAR - 9)), int(rng.integers(1, 9))
                s[a:a + k] = bytes([ch]) * k
        if i % 23 == 5:                                        # below the -A bound: 5 % of the sites are left
            s[NCHAR // 20:] = b"N" * (NCHAR - NCHAR // 20)
        if i % 7 == 3:
            s = bytearray(bytes(s).lower())
        refs[i] = bytes(s)
    names[40] = b"q3"                                          # named like a query (-x)
    cut = 170
    names.insert(100, b"short and poor"); refs.insert(100, b"N" * 400 + b"ACGT")      # too ambiguous, of another length: dropped, not fatal
    cut += 1
    accepted = sum(1 for s in refs[:cut] if sum(c not in b"NnXxOo-?." for c in s) >= int(NCHAR * (1. - 0.9)))
    assert accepted % POOL != 0 and accepted > 2 * POOL       # the first file ends in a short pool
    queries, _r, _c = F.synth_alignment(12, NCHAR, seed=32, p_snp=0.02, root=root, poly_cols=cols)
    return names, refs, cut, queries


def _totals(err):
    m = re.findall(r"Total of (\d+) sequences read; (\d+) saved sequences include closest neighbours and intermediate, (\d+) too ambiguous", err)
    x = re.findall(r" (\d+) reference sequences already present in query alignment", err)
    assert m, err[-2000:]
    return m[-1] + (x[-1] if x else "0",)


@pytest.fixture(scope="module")
def searched(tmp_path_factory):
    """every case of `uvaia` as ("default" or a label of the option's settings) -> (return code, stderr); all commands run together"""
    d = tmp_path_factory.mktemp("search_parse")
    names, refs, cut, queries = _references()
    q = d / "q.fa"
    q.write_bytes(FL.fasta([b"q%d" % i for i in range(12)], queries))
    shapes = {"plain": dict(), "wrapped": dict(wrap=60, eol=b"\r\n"), "compressed": dict(wrap=70)}
    files = {}
    for shape, kw in shapes.items():
        paths = []
        for i, (a, b) in enumerate(((0, cut), (cut, len(refs)))):
            op, suffix = ((gzip.open, ".gz"), (lzma.open, ".xz"))[i] if shape == "compressed" else (open, "")
            p = d / ("%s_%d.fa%s" % (shape, i, suffix))
            with op(p, "wb") as fh:
                fh.write(FL.fasta(names[a:b], refs[a:b], **kw))
            paths.append(str(p))
        files[shape] = paths
    good = FL.fasta(names[:50], refs[:50]) + b">short\n" + refs[50][:450] + b"\n" + FL.fasta(names[51:80], refs[51:80])
    (d / "other_good.fa").write_bytes(good)
    (d / "stray.fa").write_bytes(b"stray text\n" + FL.fasta(names[:30], refs[:30]))
    files["other_good"], files["stray"] = [str(d / "other_good.fa")], [str(d / "stray.fa")]
    small = ["--parse-block", "4096"]
    runs = [("plain", [], None), ("plain", [], small + ["--parse-window", "64"]), ("plain", [], small + ["--parse-window", "256"]), ("plain", [], small), ("plain", [], []),
            ("wrapped", [], None), ("wrapped", [], small), ("compressed", [], None), ("compressed", [], small + ["--parse-window", "64"])]
    for opt in ("-x", "--acgt", "-k"):
        runs += [("plain", [opt], None), ("plain", [opt], small + ["--parse-window", "64"])]
    runs += [("other_good", [], None), ("other_good", [], small), ("stray", [], small)]
    cmds, keys = [], []
    for shape, opts, parse in runs:
        key = (shape, " ".join(opts), "default" if parse is None else " ".join(parse))
        prefix = str(d / ("out%d" % len(keys)))
        cmd = [UVAIA, "-n", "4", "-p", str(POOL), "-A", "0.9", "-o", prefix] + opts + ([] if parse is None else ["--device-parse"] + parse)
        for f in files[shape]:
            cmd += ["-r", f]
        cmds.append(cmd + [str(q)])
        keys.append((key, prefix))
    res = _run_together(cmds)
    return {k: (p,) + r for (k, p), r in zip(keys, res)}, files


def _same_outputs(searched, shape, opts, parse):
    res, _files = searched
    pa, rca, erra = res[(shape, opts, "default")]
    pb, rcb, errb = res[(shape, opts, parse)]
    assert rca == 0, erra[-3000:]
    assert rcb == 0, errb[-3000:]
    for suffix in (".csv.xz", ".aln.xz"):
        a, b = lzma.open(pa + suffix).read(), lzma.open(pb + suffix).read()
        assert a == b, (shape, opts, parse, suffix)
        assert a.count(b"\n") > 12, (shape, opts, suffix)
    assert _totals(erra) == _totals(errb), (shape, opts, parse)
    assert re.search(r'device parse: \{"bytes": \d+, "block_bytes": \d+, "window": \d+, "scan_ms": [0-9.]+, "rows_ms": [0-9.]+, "text_in_ms": [0-9.]+, "text_out_ms": [0-9.]+\}', errb), errb[-1000:]
    return errb


def test_blocks_and_windows_give_the_files_of_the_default_route(searched):
    windows = {}
    for parse in ("--parse-block 4096 --parse-window 64", "--parse-block 4096 --parse-window 256", "--parse-block 4096", ""):
        err = _same_outputs(searched, "plain", "", parse)
        windows[parse] = int(re.search(r'"window": (\d+)', err).group(1))
    assert windows["--parse-block 4096 --parse-window 64"] == 64 and windows["--parse-block 4096 --parse-window 256"] == 256
    assert windows[""] == 65536 and windows["--parse-block 4096"] == 65536          # the default: the smallest multiple of the pool from 65 536 on
    totals = _totals(searched[0][("plain", "", "")][2])
    assert int(totals[0]) == 301 and int(totals[2]) >= 13                            # every record was counted, the short one among the ambiguous


def test_wrapped_and_compressed_text(searched):
    _same_outputs(searched, "wrapped", "", "--parse-block 4096")
    _same_outputs(searched, "compressed", "", "--parse-block 4096 --parse-window 64")
    res = searched[0]
    for suffix in (".csv.xz", ".aln.xz"):                                            # ... which is also what the plain text gives
        assert lzma.open(res[("wrapped", "", "--parse-block 4096")][0] + suffix).read() == lzma.open(res[("plain", "", "default")][0] + suffix).read()


@pytest.mark.parametrize("opt", ["-x", "--acgt", "-k"])
def test_with_the_options_of_the_search(searched, opt):
    err = _same_outputs(searched, "plain", opt, "--parse-block 4096 --parse-window 64")
    if opt == "-x":
        assert _totals(err)[3] == "1"


def test_what_ends_the_command(searched):
    res = searched[0]
    for how in ("default", "--parse-block 4096"):                                    # a well-resolved record of another length: both routes end
        _p, rc, err = res[("other_good", "", how)]
        assert rc != 0 and "all sequences must be aligned" in err and "'short'" in err, (how, err[-2000:])
    _p, rc, err = res[("stray", "", "--parse-block 4096")]                           # irregular text: the file, the offset and the way back
    assert rc != 0 and "stray.fa: FASTA text:" in err and "at byte 0 of the text" in err and "`uvaia` without it reads this file line by line" in err, err[-2000:]


# ------------------------------------------------------------------------------------------------------------------ uvaiaclust
@pytest.fixture(scope="module")
def clustered(tmp_path_factory):
    """`uvaiaclust -d 3 -p 8` over the same references in two files, without the option and with it, as (prefix, return code, stderr)"""
    d = tmp_path_factory.mktemp("clust_parse")
    names, refs, cut, _q = _references()
    keep = [i for i, s in enumerate(refs) if len(s) == NCHAR]
    cut = sum(1 for i in keep if i < cut)
    names, refs = [names[i] for i in keep], [refs[i] for i in keep]
    shapes = {"plain": dict(), "wrapped": dict(wrap=60, eol=b"\r\n"), "compressed": dict(wrap=70)}
    files = {}
    for shape, kw in shapes.items():
        paths = []
        for i, (a, b) in enumerate(((0, cut), (cut, len(refs)))):
            op, suffix = ((gzip.open, ".gz"), (lzma.open, ".xz"))[i] if shape == "compressed" else (open, "")
            p = d / ("%s_%d.fa%s" % (shape, i, suffix))
            with op(p, "wb") as fh:
                fh.write(FL.fasta(names[a:b], refs[a:b], **kw))
            paths.append(str(p))
        files[shape] = paths
    (d / "other.fa").write_bytes(FL.fasta(names[:20], refs[:20]) + b">short\n" + refs[20][:450] + b"\n")
    high = refs[5][:77] + b"\xc3" + refs[5][78:]
    (d / "high.fa").write_bytes(FL.fasta(names[:5] + [b"high byte"], refs[:5] + [high]))
    files["other"], files["high"] = [str(d / "other.fa")], [str(d / "high.fa")]
    small = ["--device-parse", "--parse-block", "4096"]
    runs = {("plain", "default"): ("plain", []), ("plain", "parse"): ("plain", small), ("plain", "parse_default_block"): ("plain", ["--device-parse"]),
            ("keep", "default"): ("plain", ["--keep-medoids"]), ("keep", "parse"): ("wrapped", ["--keep-medoids"] + small),
            ("out", "default"): ("plain", ["--packed-out", "@.uvdb"]), ("out", "parse"): ("compressed", ["--packed-out", "@.uvdb"] + small),
            ("compact", "default"): ("plain", ["--packed-out", "@.uvdb", "--compact"]), ("compact", "parse"): ("plain", ["--packed-out", "@.uvdb", "--compact", "--keep-medoids"] + small),
            ("other", "default"): ("other", []), ("other", "parse"): ("other", small), ("high", "default"): ("high", []), ("high", "parse"): ("high", small)}
    cmds, keys = [], []
    for key, (shape, opts) in runs.items():
        prefix = str(d / ("clust%d" % len(keys)))
        cmds.append([UVAIACLUST, "-d", "3", "-p", "8", "-o", prefix] + [o.replace("@", prefix) for o in opts] + files[shape])
        keys.append((key, prefix))
    res = _run_together(cmds)
    return {k: (p,) + r for (k, p), r in zip(keys, res)}


@pytest.mark.parametrize("case,how", [("plain", "parse"), ("plain", "parse_default_block"), ("keep", "parse"), ("out", "parse"), ("compact", "parse")])
def test_uvaiaclust_writes_the_files_of_the_default_route(clustered, case, how):
    pa, rca, erra = clustered[(case, "default")]
    pb, rcb, errb = clustered[(case, how)]
    assert rca == 0, erra[-3000:]
    assert rcb == 0, errb[-3000:]
    for suffix in (".csv.xz", ".aln.xz"):
        a, b = lzma.open(pa + suffix).read(), lzma.open(pb + suffix).read()
        assert a == b and a.count(b"\n") > 3, (case, suffix)
    if case in ("out", "compact"):
        assert filecmp.cmp(pa + ".uvdb", pb + ".uvdb", shallow=False), case
    count = lambda e: re.search(r"(\d+) clusters from (\d+) sequences", e).groups()
    assert count(erra) == count(errb) and count(errb)[1] == "300"
    assert re.search(r'device parse: \{"bytes": \d+, "block_bytes": \d+, "scan_ms": [0-9.]+, "rows_ms": [0-9.]+, "rows_in_ms": [0-9.]+\}', errb), errb[-1000:]


def test_uvaiaclust_ends_where_the_default_route_ends(clustered):
    for how in ("default", "parse"):
        _p, rc, err = clustered[("other", how)]              # a record of another length: today's message
        assert rc != 0 and "cannot work with unaligned sequences; sequence short has 450 sites while reference has 600" in err, (how, err[-2000:])
        _p, rc, err = clustered[("high", how)]               # a bad byte: reported with the sequence's name
        assert rc != 0 and "sequence high byte holds byte 0xc3 at site 78: only bytes 1-127 are defined" in err, (how, err[-2000:])
