"""The pair counters of uvaia_gpu_db_pairs without a GPU: the plane formulas of include/uvaia_gpu.h, restated in numpy over the packed
tiles, give what the oracle's two kernels give over the trimmed text; the reference README's toy example gives the README's numbers; and
what `uvaiadist` refuses before any device work."""
import os
import subprocess

import numpy as np
import pytest

import pair_dist as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIADIST = os.path.join(ROOT, "bin", "uvaiadist")


@pytest.mark.parametrize("name", D.CPU_CASES)
def test_plane_formulas_equal_the_oracle(name):
    seqs, nchar = D.case(name)
    for trim in D.trims_of(nchar):
        got = D.plane_counts_of(seqs, nchar, trim)
        assert np.array_equal(got, D.oracle_counts(name, trim)), (name, trim)
        if 2 * trim == nchar:
            assert not got.any()


def test_counters_are_symmetric_and_the_diagonal_is_at_distance_zero():
    c = D.oracle_counts("synth130", 0)
    assert np.array_equal(c, c.transpose(1, 0, 2))
    assert not np.diagonal(D.snp(c)).any() and not np.diagonal(D.uvaia(c)).any()


def test_readme_toy_example():
    """reference README lines 307-316: the three pairs of AACGTTA-- / AACG-TAM- / MNCGTTMC- have ACGT_matches 6, 4, 3, partial_matches 6, 6, 6
    and valid_pair_comparisons 6, 6, 6 (reference-produced numbers)"""
    seqs = list(D.README_TOY)
    pairs = ((0, 1), (0, 2), (1, 2))
    for counts in (D.oracle_counts_of(seqs), D.plane_counts_of(seqs, 9)):
        assert [int(counts[i, j, 0]) for i, j in pairs] == [6, 4, 3]
        assert [int(counts[i, j, 2]) for i, j in pairs] == [6, 6, 6]
        assert [int(counts[i, j, 3]) for i, j in pairs] == [6, 6, 6]
        assert [int(D.uvaia(counts)[i, j]) for i, j in pairs] == [0, 0, 0]


def test_threshold_cases_are_neither_empty_nor_everything():
    c = D.oracle_counts("synth130", 0)
    assert [len(D.within_expected(c, d)) for d in (0, 1, 2)] == [1561, 4441, 6777]
    assert 130 * 129 // 2 == 8385


# ---- uvaiadist: what is refused before any device work
def run(*args):
    return subprocess.run([UVAIADIST, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_help_exits_zero():
    r = run("-h")
    assert r.returncode == 0 and b"uvaiadist" in r.stdout + r.stderr


@pytest.mark.parametrize("args, message", [
    (("--metric=hamming", "--stdout", "x.fa"), b"unknown metric"),
    (("--long", "--counts", "--stdout", "x.fa"), b"--long and --counts"),
    (("-d", "2", "--stdout", "--dense", "x.fa"), b"-d needs a long form"),
    (("--stdout", "--packed", "a.uvdb", "x.fa"), b"cannot be mixed"),
    (("x.fa",), b"-o <file> or --stdout"),
    (("-o", "out.tsv", "--stdout", "x.fa"), b"both -o and --stdout"),
])
def test_refusals_need_no_gpu(args, message):
    r = run(*args)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
