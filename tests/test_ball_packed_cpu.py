"""Host-side pieces of `uvaiaball --packed` that need no GPU: the exception pass split out of uvdb_unpack_reference, the rule that
says whether a packed file can answer a radius search exactly, and the two new entries of the C ABI."""
import os
import subprocess

import pytest

import packed_lib as P
from uvaia_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nchar", [29, 333, 1000])          # below one word, not a multiple of 32 or 128, a multiple of neither
def test_apply_exceptions_is_the_second_half_of_unpack_reference(tmp_path, nchar):
    seqs = P.awkward_references(70, nchar, seed=5 + nchar)   # two tiles, the second one partial
    upper = [s.upper() for s in seqs]
    names = ["ref/%d|x" % i for i in range(len(seqs))]
    planes, non_n = P.pack_tiles(seqs, nchar)
    P.write_uvdb(tmp_path / "db.uvdb", names, upper, planes, non_n)
    r = P.Reader(tmp_path / "db.uvdb", nchar)
    try:
        n_exc = 0
        for i in range(len(seqs)):
            whole = r.unpack_reference(i)
            assert whole == upper[i], i
            bare = P.decode_reference(planes, i, nchar)      # what a decoder of the planes alone gives: N at every invalid site
            assert bare == bytes(ord("N") if c in P.EXCEPTIONS else c for c in upper[i]), i
            assert r.apply_exceptions(i, bare) == whole, i
            n_exc += bare != whole
        assert n_exc > len(seqs) // 2                        # the set does exercise the pass
        assert r.apply_exceptions(len(seqs), b"A" * nchar) == b"A" * nchar      # outside the file: the row is left alone
    finally:
        r.close()


# (nchar, -A of the radius search, -A of the packing, exact?): (int)(nchar * A) >= (int)(nchar * (1 - A_pack)), worked out by hand
FILTER_TABLE = [
    (29903, 0.5, 0.5, 1),        # 14951 >= 14951: both defaults
    (29903, 0.7, 0.5, 1),        # 20932 >= 14951
    (29903, 0.3, 0.5, 0),        #  8970 <  14951
    (29903, 0.5, 0.6, 1),        # 14951 >= 11961
    (29903, 0.5, 0.4, 0),        # 14951 <  17941
    (29903, 0.001, 0.5, 0),      # the clamps:    29 <  14951
    (29903, 1.0, 0.5, 1),        #             29903 >= 14951
    (29903, 0.5, 0.001, 0),      #             14951 <  29873
    (29903, 1.0, 0.001, 1),      #             29903 >= 29873
    (29903, 0.001, 1.0, 1),      #                29 >= 0: the file holds everything
    (100, 0.5, 0.5, 1),          #    50 >= 50
    (101, 0.5, 0.5, 1),          #    50 >= 50 (both truncate 50.5)
    (10, 0.45, 0.5, 0),          #     4 <  5
    (10, 0.55, 0.5, 1),          #     5 >= 5
]


@pytest.mark.parametrize("nchar,a_ball,a_pack,want", FILTER_TABLE)
def test_radius_filter_rule(nchar, a_ball, a_pack, want):
    assert P.radius_filter_is_exact(nchar, a_ball, a_pack) == want


def test_new_abi_entries_are_exported_and_plain_c(tmp_path):
    capi.build_library()
    lib = capi.load_library()
    for name in ("uvaia_gpu_ball_packed", "uvaia_gpu_unpack_rows"):
        assert name in capi.SYMBOLS
        assert hasattr(lib, name), name
    src = tmp_path / "t.c"
    src.write_text('#include "uvaia_gpu.h"\n'
                   "int (*search) (uvaia_gpu_ctx *, const void *, int, int, int *) = uvaia_gpu_ball_packed;\n"
                   "int (*text) (uvaia_gpu_ctx *, const int *, int, char *, size_t) = uvaia_gpu_unpack_rows;\n"
                   "int main (void) { return search == 0 || text == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_uvaiaball_refuses_before_it_needs_a_gpu(tmp_path):
    """the option and filter checks of `uvaiaball --packed` come before the engine is opened: a file written here (no GPU) is enough"""
    import fixtures as F
    from uvaia_amd import hostlib
    hostlib.build_library()
    ball = os.path.join(ROOT, "bin", "uvaiaball")
    nchar = 400
    root = F.random_acgt(nchar, 5)
    refs = [root] * 70
    planes, non_n = P.pack_tiles(refs, nchar)
    db = str(tmp_path / "r.uvdb")
    P.write_uvdb(db, ["r%d" % i for i in range(len(refs))], refs, planes, non_n, ref_ambiguity=0.5)
    q = tmp_path / "q.fa"
    q.write_bytes(b">q0\n" + root + b"\n>q1\n" + root[:10] + (b"A" if root[10:11] != b"A" else b"C") + root[11:] + b"\n")
    for extra, word in ((["-A", "0.3"], b"packed"), (["-r", str(q)], b"")):          # a filter the file cannot honour; -r next to --packed
        cmd = [ball, str(q), "-o", str(tmp_path / "out"), "--packed", db] + extra
        r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode != 0 and word in r.stderr, cmd
        assert b"HIP device" not in r.stderr, cmd            # refused on its own grounds, not for the missing GPU
    r = subprocess.run([ball, "-r", str(q), "--devices", "0,0", str(q), "-o", str(tmp_path / "out")], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and b"--packed" in r.stderr
