"""`uvaiaclust --packed` without a GPU: the new entries of the C ABI are exported and the header stays plain C; the command line refuses a
damaged database, --packed next to alignment files and a -r reference of another length on its own grounds, before it needs a device."""
import os
import re
import subprocess

import pytest

import fixtures as F
import packed_lib as P
from uvaia_amd import capi, cluster, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")
NEW = ("uvaia_clust_push_packed", "uvaia_clust_rows", "uvaia_clust_device_rows", "uvaia_clust_unpack_ms")


def test_every_declared_function_is_exported():
    capi.build_library()
    lib = capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "uvaia_cluster.h")).read()
    declared = set(re.findall(r"\b(uvaia_clust_[a-z_0-9]+)\s*\(", hdr))
    assert set(NEW) <= declared
    assert declared == set(cluster.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name


def test_header_is_plain_c_with_the_new_signatures(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "uvaia_cluster.h"\n'
                   "int (*push) (uvaia_clust_ctx *, int, const void *, const uint64_t *, const void *, const int *) = uvaia_clust_push_packed;\n"
                   "int (*rows) (uvaia_clust_ctx *, const int64_t *, int, char *, size_t) = uvaia_clust_rows;\n"
                   "int (*where) (uvaia_clust_ctx *, const void **, size_t *) = uvaia_clust_device_rows;\n"
                   "int (*ms) (uvaia_clust_ctx *, double *, double *) = uvaia_clust_unpack_ms;\n"
                   "int (*stats) (uvaia_clust_ctx *, double *, double *, double *, int64_t *) = uvaia_clust_stats;\n"
                   "int main (void) { return push == 0 || rows == 0 || where == 0 || ms == 0 || stats == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


@pytest.fixture(scope="module")
def database(tmp_path_factory):
    """a small valid database written here (no GPU): 70 references of 400 sites, some with exception runs"""
    hostlib.build_library()
    d = tmp_path_factory.mktemp("clust_packed_cpu")
    nchar = 400
    seqs = [s.upper() for s in P.awkward_references(70, nchar, seed=11)]
    planes, non_n = P.pack_tiles(seqs, nchar)
    path = str(d / "in.uvdb")
    P.write_uvdb(path, ["ref/%d" % i for i in range(len(seqs))], seqs, planes, non_n, ref_ambiguity=1.0)
    return d, path, nchar


def _run(args):
    r = subprocess.run([UVAIACLUST] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return r.returncode, (r.stdout + r.stderr).decode(errors="replace")


def _refused_on_its_own_grounds(code, text):
    assert code != 0, text
    assert "HIP device" not in text and "gfx950" not in text, text      # not for the missing GPU


def test_truncated_database_is_refused(database):
    d, path, _ = database
    blob = open(path, "rb").read()
    cut = str(d / "cut.uvdb")
    open(cut, "wb").write(blob[:len(blob) - 100])
    code, text = _run(["--packed", cut, "-o", str(d / "o1")])
    _refused_on_its_own_grounds(code, text)
    assert "truncated or inconsistent" in text
    assert not (d / "o1.csv.xz").exists()


def test_corrupted_database_is_refused(database):
    d, path, _ = database
    blob = bytearray(open(path, "rb").read())
    blob[0:4] = b"XXXX"                                                  # the magic
    bad = str(d / "magic.uvdb")
    open(bad, "wb").write(bytes(blob))
    code, text = _run(["--packed", bad, "-o", str(d / "o2")])
    _refused_on_its_own_grounds(code, text)
    assert "not a packed uvaia database" in text
    blob = bytearray(open(path, "rb").read())
    blob[12:16] = (4000).to_bytes(4, "little")                           # nchar no longer fits W4 and the tile size
    bad = str(d / "nchar.uvdb")
    open(bad, "wb").write(bytes(blob))
    code, text = _run(["--packed", bad, "-o", str(d / "o3")])
    _refused_on_its_own_grounds(code, text)
    assert "truncated or inconsistent" in text


def test_packed_next_to_alignment_files_is_a_usage_error(database):
    d, path, nchar = database
    fa = d / "a.fa"
    fa.write_bytes(b">s1\n" + F.random_acgt(nchar, 3) + b"\n")
    code, text = _run(["--packed", path, "-o", str(d / "o4"), str(fa)])
    _refused_on_its_own_grounds(code, text)
    assert "--packed" in text and "not both" in text
    assert not (d / "o4.csv.xz").exists()
    code, text = _run(["-o", str(d / "o5")])                             # neither: the usage error it has always been
    assert code != 0 and "The complete syntax is" in text


def test_reference_of_another_length_is_refused(database):
    d, path, nchar = database
    ref = d / "ref.fa"
    ref.write_bytes(b">ref\n" + F.random_acgt(nchar - 1, 4) + b"\n")
    code, text = _run(["--packed", path, "-r", str(ref), "-o", str(d / "o6")])
    _refused_on_its_own_grounds(code, text)
    assert "unaligned" in text and str(nchar - 1) in text and str(nchar) in text
    assert not (d / "o6.csv.xz").exists()


def test_help_lists_the_new_options():
    code, text = _run(["--help"])
    assert code == 0
    for word in ("--packed=", "--packed-out=", "-A, --ref_ambiguity"):
        assert word in text, word
